// nrx_train.hip -- training of the CGNN: f32 forward with kept activations, the loss of include/nrx.h
// (nrx_train_io), the backward pass and the Adam update.  Nothing here is shared with the inference kernels
// (f16, fused, no activations kept).
//
// Layout: every activation and every gradient of an activation is position-major, [P][C] f32 with
// P = B U F 14 positions p = ((b U + u) F + f) 14 + t, so that every 1x1 convolution and every dense layer is
// one of three GEMM shapes over positions, all on the exact-f32 MFMA v_mfma_f32_32x32x2_f32:
//   k_gemm   forward        Y = X W + b (+ residual) (ReLU)                  [P x K] [K x N]
//            backward-data  dX = dZ W^T, zeroed where the stored ReLU output is 0, optionally added to dX
//                           (the same kernel: the B operand is read with swapped strides)
//   k_wgrad  backward-weight  dW = X^T dZ and db = column sums of dZ: each workgroup reduces its chunk of
//                           positions into one [K + 1][N] slab (plain stores), k_slab_sum adds the slabs in
//                           their fixed order (in f64) onto grad.  No atomics: bit-reproducible.
// The depthwise 3x3 (SAME, zero outside the grid, nothing crosses a (slot, user)) is VALU work: k_dw forward and
// backward-data (flipped taps), k_dwgrad the [9][C] tap gradient, slabs as above.  Its output D is stored, not
// recomputed.  The rest is elementwise: k_z0 ([y ns, pe, h ns]), k_rowscale (the per-MCS StateInit sum and its
// transpose), k_concat / k_concat_bwd ([a, s, pe] with the leave-one-out user mean, no gradient into pe, and the
// skip connection's gradient), k_loss_llr / k_loss_chest (loss terms summed in f64 per workgroup in a fixed
// order, and the derivative at the heads), k_loss_sum.
//
// Workspace, floats per position (H LLR heads / StateInit stacks, I = num_it, R readouts = I with multiloss, else
// 1, c0 = StateInit input width (2 or 4) A + 2, hb_h = width of head h):
//   z0 c0;  per StateInit stack  c0 + 4 x 128;  states (I + 1) x 56
//   per iteration  64 + 56 + 114 + 114 + 4 x 128 = 860
//   per readout    sum_h (128 + 2 hb_h) + 128 + 4 A
//   gradients      2 x 128 + 3 x 56 + 64 = 488 (two hidden-width buffers, dS, the aggregate's, the masked state's)
// plus the weight-gradient slabs (S <= 256 chunks of positions, S x 129 x 128 floats), the loss partials and the
// slot norms; every piece rounded up to 256 bytes.  nrx_rt (A = 4, h_hat, I = 2, one 4-bit head): 18 + 530 + 168
// + 1720 + 280 + 488 = 3204 floats = 12816 bytes per position without multiloss.
#include <hip/hip_runtime.h>

#include <vector>

#include "nrx_internal.h"
#include "nrx_model.h"

namespace nrx {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kTB = 256;          // threads of every workgroup here
constexpr int kLossBlocks = 256;  // workgroups (= f64 partials) of one loss launch
constexpr int kMaxSlabs = 256;
constexpr int kLd = 160;          // LDS row of 128 floats + 32: the two k rows of an MFMA read hit different banks

// ---------------------------------------------------------------- GEMM over positions
struct GemmArgs {
  const float* A; int lda;          // [P][K]
  const float* W; int sbk, sbj;     // B[k][j] = W[k sbk + j sbj]
  const float* bias;                // [N] or null
  const float* res; int ldr;        // added to the result, or null
  const float* mask; int ldm;       // result zeroed where mask <= 0 (a stored ReLU output), or null
  float* C; int ldc;                // [P][N]
  int P, K, N, relu, accumulate;
};

// 128 positions x (N <= 128) per workgroup; wave w owns rows [32 w, 32 w + 32) and every 32-column tile.  K in
// chunks of 32 through LDS; rows beyond P, k beyond K and columns beyond N are zero in LDS, never read in memory.
__global__ __launch_bounds__(kTB) void k_gemm(GemmArgs g) {
  __shared__ float As[128][33];
  __shared__ float Bs[32][kLd];
  const int t = threadIdx.x, w = t >> 6, l = t & 63, r = l & 31, h = l >> 5;
  const int p0 = blockIdx.x * 128;
  const int nct = (g.N + 31) >> 5;
  f32x16 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
  for (int k0 = 0; k0 < g.K; k0 += 32) {
    {
      const int c = t & 31, k = k0 + c;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (t >> 5) + 8 * i, p = p0 + row;
        As[row][c] = (p < g.P && k < g.K) ? g.A[(size_t)p * g.lda + k] : 0.f;
      }
      const int j = t & 127;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kr = (t >> 7) + 2 * i, kk = k0 + kr;
        Bs[kr][j] = (kk < g.K && j < g.N) ? g.W[(size_t)kk * g.sbk + (size_t)j * g.sbj] : 0.f;
      }
    }
    __syncthreads();
    const int kend = min(32, (g.K - k0 + 1) & ~1);
    for (int kk = 0; kk < kend; kk += 2) {
      const float a = As[32 * w + r][kk + h];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < nct) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[kk + h][32 * c + r], acc[c], 0, 0, 0);
    }
    __syncthreads();
  }
  // C / D layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = 32 * c + r;
    if (c >= nct || col >= g.N) continue;
    const float b = g.bias ? g.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int p = p0 + 32 * w + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (p >= g.P) continue;
      float v = acc[c][i] + b;
      if (g.res) v += g.res[(size_t)p * g.ldr + col];
      if (g.relu) v = fmaxf(v, 0.f);
      if (g.mask && !(g.mask[(size_t)p * g.ldm + col] > 0.f)) v = 0.f;
      float* out = g.C + (size_t)p * g.ldc + col;
      *out = g.accumulate ? *out + v : v;
    }
  }
}

// ---------------------------------------------------------------- weight gradient: X^T dZ and the bias sum
struct WgradArgs {
  const float* X; int ldx;   // [P][K]
  const float* Z; int ldz;   // [P][N]
  float* slab;               // [S][(K + 1) N]: rows k < K = X^T Z, row K = column sums of Z
  int P, K, N, PC;           // PC positions (a multiple of 32) per workgroup
};

// workgroup s reduces positions [s PC, (s + 1) PC) in steps of 32; wave w owns the weight rows [32 w, 32 w + 32)
__global__ __launch_bounds__(kTB) void k_wgrad(WgradArgs g) {
  __shared__ float Xs[32][kLd];
  __shared__ float Zs[32][kLd];
  const int t = threadIdx.x, w = t >> 6, l = t & 63, r = l & 31, h = l >> 5;
  const int pb = blockIdx.x * g.PC, pe = min(g.P, pb + g.PC);
  const int nct = (g.N + 31) >> 5, nrt = (g.K + 31) >> 5;
  f32x16 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
  float bsum = 0.f;
  for (int p0 = pb; p0 < pe; p0 += 32) {
    const int col = t & 127;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = (t >> 7) + 2 * i, p = p0 + row;
      Xs[row][col] = (p < pe && col < g.K) ? g.X[(size_t)p * g.ldx + col] : 0.f;
      Zs[row][col] = (p < pe && col < g.N) ? g.Z[(size_t)p * g.ldz + col] : 0.f;
    }
    __syncthreads();
    if (t < g.N)
      for (int i = 0; i < 32; ++i) bsum += Zs[i][t];
    if (w < nrt)
      for (int kk = 0; kk < 32; kk += 2) {
        const float a = Xs[kk + h][32 * w + r];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < nct) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Zs[kk + h][32 * c + r], acc[c], 0, 0, 0);
      }
    __syncthreads();
  }
  float* slab = g.slab + (size_t)blockIdx.x * (g.K + 1) * g.N;
  if (t < g.N) slab[(size_t)g.K * g.N + t] = bsum;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = 32 * c + r;
    if (c >= nct || col >= g.N) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int k = 32 * w + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (k < g.K) slab[(size_t)k * g.N + col] = acc[c][i];
    }
  }
}

// grad[e] += sum over the S slabs, in slab order, in f64 (grad was zeroed at the start of the call, or holds
// the sum of the calls before this one when the call accumulates)
__global__ void k_slab_sum(const float* slab, int S, int n, float* grad) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int i = 0; i < S; ++i) s += (double)slab[(size_t)i * n + e];
  grad[e] = (float)((double)grad[e] + s);
}

// ---------------------------------------------------------------- depthwise 3x3
// forward: out[p][c] = sum_ij w[i][j][c] x[f + i - 1][t + j - 1][c]; BWD: the correlation with the flipped taps,
// out[p][c] = sum_ij w[i][j][c] x[f - i + 1][t - j + 1][c], zeroed where mask <= 0 (mask: the layer's input, a
// stored ReLU output, or null)
template <bool BWD>
__global__ void k_dw(const float* x, int ldx, const float* w, int C, float* out, int ldo, const float* mask, int ldm,
                     int F, int P) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)P * C) return;
  const int p = (int)(idx / C), c = (int)(idx % C);
  const int rr = p % (F * kT), f = rr / kT, t = rr % kT;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int df = BWD ? 1 - i : i - 1, dt = BWD ? 1 - j : j - 1;
      if (f + df < 0 || f + df >= F || t + dt < 0 || t + dt >= kT) continue;
      acc = fmaf(w[(i * 3 + j) * C + c], x[(size_t)(p + df * kT + dt) * ldx + c], acc);
    }
  if (mask && !(mask[(size_t)p * ldm + c] > 0.f)) acc = 0.f;
  out[(size_t)p * ldo + c] = acc;
}

// tap gradient: slab[s][tap][c] = sum over the positions of chunk s of x[p + tap][c] dD[p][c]; thread = channel
__global__ __launch_bounds__(128) void k_dwgrad(const float* x, int ldx, const float* dD, int ldd, int C, int F,
                                                 int P, int PC, float* slab) {
  const int c = threadIdx.x;
  if (c >= C) return;
  const int pb = blockIdx.x * PC, pe = min(P, pb + PC);
  float acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.f;
  for (int p = pb; p < pe; ++p) {
    const int rr = p % (F * kT), f = rr / kT, t = rr % kT;
    const float d = dD[(size_t)p * ldd + c];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (f + i - 1 < 0 || f + i - 1 >= F || t + j - 1 < 0 || t + j - 1 >= kT) continue;
        acc[i * 3 + j] = fmaf(x[(size_t)(p + (i - 1) * kT + (j - 1)) * ldx + c], d, acc[i * 3 + j]);
      }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) slab[((size_t)blockIdx.x * 9 + k) * C + c] = acc[k];
}

// ---------------------------------------------------------------- elementwise pieces
// sum of 256 doubles, one per thread, in a fixed tree; the result in thread 0
__device__ double block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = kTB / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

// per-slot scale 1 / sqrt(mean y^2) (0 for an all-zero slot); one workgroup per slot
__global__ __launch_bounds__(kTB) void k_norm(const float* y, int n, float* ns) {
  __shared__ double sh[kTB];
  const float* yb = y + (size_t)blockIdx.x * n;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kTB) s += (double)yb[i] * (double)yb[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    const double ms = s / n;
    ns[blockIdx.x] = ms > 0.0 ? (float)(1.0 / sqrt(ms)) : 0.f;
  }
}

// StateInit input z0[p] = [y[b, f, t] ns_b (2A), pe[u, f, t] (2), h_hat[p] ns_b (2A, with h_hat)]
__global__ void k_z0(const float* y, const float* pe, const float* hh, const float* ns, int U, int F, int A2, int C0,
                     int P, float* z0) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)P * C0) return;
  const int p = (int)(idx / C0), c = (int)(idx % C0);
  const int FT = F * kT, bu = p / FT, rr = p % FT, b = bu / U, u = bu % U;
  float v;
  if (c < A2) v = y[((size_t)b * FT + rr) * A2 + c] * ns[b];
  else if (c < A2 + 2) v = pe[((size_t)u * FT + rr) * 2 + (c - A2)];
  else v = hh[(size_t)p * A2 + (c - A2 - 2)] * ns[b];
  z0[idx] = v;
}

// dst[p][c] (+)= scale[b, u] src[p][c], scale = mcs_mask[b, u, m] (null mask: one-hot on MCS 0)
__global__ void k_rowscale(const float* src, const float* mask, int M, int m, int FT, int C, int P, int accumulate,
                           float* dst) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)P * C) return;
  const int bu = (int)(idx / C) / FT;
  const float sc = mask ? mask[(size_t)bu * M + m] : (m == 0 ? 1.f : 0.f);
  const float v = sc * src[idx];
  dst[idx] = accumulate ? dst[idx] + v : v;
}

__device__ float loo_factor(const float* active, int b, int U) {
  float n = 0.f;
  for (int u = 0; u < U; ++u) n += active[b * U + u];
  n = fmaxf(n - 1.f, 0.f);
  return n == 0.f ? 1.f : 1.f / n;
}

// zcat[p] = [a (56), s (56), pe (2)], a[b, u] = factor_b sum over u' != u of active[b, u'] sp[b, u']
__global__ void k_concat(const float* sp, const float* s, const float* pe, const float* active, int U, int F, int P,
                         float* zcat) {
  constexpr int C = 2 * kDS + 2;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)P * C) return;
  const int p = (int)(idx / C), c = (int)(idx % C);
  const int FT = F * kT, bu = p / FT, rr = p % FT, b = bu / U, u = bu % U;
  float v;
  if (c < kDS) {
    float acc = 0.f;
    for (int o = 0; o < U; ++o)
      if (o != u) acc += active[b * U + o] * sp[((size_t)(b * U + o) * FT + rr) * kDS + c];
    v = acc * loo_factor(active, b, U);
  } else if (c < 2 * kDS) {
    v = s[(size_t)p * kDS + (c - kDS)];
  } else {
    v = pe[((size_t)u * FT + rr) * 2 + (c - 2 * kDS)];
  }
  zcat[idx] = v;
}

// the transpose: dsp[b, u] = active[b, u] factor_b sum over u' != u of da[b, u'], and the state's own share
// dS[p] += dz[p][56..112) (the skip connection's share is what dS already holds)
__global__ void k_concat_bwd(const float* dz, int ldz, const float* active, int U, int F, int P, float* dS,
                             float* dsp) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)P * kDS) return;
  const int p = (int)(idx / kDS), c = (int)(idx % kDS);
  const int FT = F * kT, bu = p / FT, rr = p % FT, b = bu / U, u = bu % U;
  float acc = 0.f;
  for (int o = 0; o < U; ++o)
    if (o != u) acc += dz[((size_t)(b * U + o) * FT + rr) * ldz + c];
  dsp[idx] = active[b * U + u] * loo_factor(active, b, U) * acc;
  dS[idx] += dz[(size_t)p * ldz + kDS + c];
}

// dst[p][0..nd) = src[p][0..ns), zero beyond: the caller's llr tensor has rows of bits_max
__global__ void k_copy_cols(const float* src, int ns, float* dst, int nd, int P) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)P * nd) return;
  const int p = (int)(idx / nd), c = (int)(idx % nd);
  dst[idx] = c < ns ? src[(size_t)p * ns + c] : 0.f;
}

// ---------------------------------------------------------------- loss and its derivative at the heads
struct LossLlrArgs {
  const float* llr;            // [P][hb]
  const uint8_t* bits; int bits_stride;
  const float* active;         // [B U]
  const float* mask; int M;    // [B U][M] or null
  int m_lo, m_hi;              // the MCS this head serves
  int bits_m[8];
  double inv_den[8];           // 1 / (B U F (14 - n_dmrs) bits_m)
  int dmrs_mask, hb, FT, P;
  float* dllr;                 // [P][hb]
  double* part;                // [kLossBlocks]
};

__global__ __launch_bounds__(kTB) void k_loss_llr(LossLlrArgs g) {
  __shared__ double sh[kTB];
  double sum = 0.0;
  const size_t n = (size_t)g.P * g.hb;
  for (size_t idx = (size_t)blockIdx.x * kTB + threadIdx.x; idx < n; idx += (size_t)kLossBlocks * kTB) {
    const int p = (int)(idx / g.hb), k = (int)(idx % g.hb), bu = p / g.FT, t = p % kT;
    double coef = 0.0;
    if (!((g.dmrs_mask >> t) & 1)) {
      const float act = g.active[bu];
      for (int m = g.m_lo; m < g.m_hi; ++m)
        if (k < g.bits_m[m])
          coef += (double)(act * (g.mask ? g.mask[(size_t)bu * g.M + m] : (m == 0 ? 1.f : 0.f))) * g.inv_den[m];
    }
    float d = 0.f;
    if (coef != 0.0) {
      const float z = g.llr[idx], bit = (float)g.bits[(size_t)p * g.bits_stride + k];
      const float e = expf(-fabsf(z));
      sum += coef * (double)(fmaxf(z, 0.f) - bit * z + log1pf(e));
      // sigmoid(z) - bit without the cancellation at a confident, correct LLR: for bit 1 it is -sigmoid(-z)
      const float big = 1.f / (1.f + e), small = e / (1.f + e);
      d = (float)coef * (bit != 0.f ? -(z >= 0.f ? small : big) : (z >= 0.f ? big : small));
    }
    g.dllr[idx] = d;
  }
  sum = block_sum(sum, sh);
  if (threadIdx.x == 0) g.part[blockIdx.x] = sum;
}

// loss terms active (h_ref - h)^2 / (P 2A); dh = w_chest 2 active (h_ref - h) / (P 2A)
__global__ __launch_bounds__(kTB) void k_loss_chest(const float* href, const float* h, const float* active, int FT,
                                                     int A2, int P, double inv_den, double w_chest, float* dh,
                                                     double* part) {
  __shared__ double sh[kTB];
  double sum = 0.0;
  const size_t n = (size_t)P * A2;
  for (size_t idx = (size_t)blockIdx.x * kTB + threadIdx.x; idx < n; idx += (size_t)kLossBlocks * kTB) {
    const int p = (int)(idx / A2);
    const float act = active[p / FT], e = href[idx] - h[idx];
    sum += (double)(act * e * e) * inv_den;
    dh[idx] = (float)(2.0 * w_chest * inv_den) * (act * e);
  }
  sum = block_sum(sum, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// loss[0] = the nd data launches' partials, loss[1] = the nc chest launches', each column of launches summed in
// launch order, then the fixed tree; with `accumulate` the two sums are added onto what loss holds
__global__ __launch_bounds__(kTB) void k_loss_sum(const double* pd, int nd, const double* pc, int nc, int accumulate,
                                                   double* loss) {
  __shared__ double sh[kTB];
  double s = 0.0;
  for (int i = 0; i < nd; ++i) s += pd[(size_t)i * kLossBlocks + threadIdx.x];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) loss[0] = accumulate ? loss[0] + s : s;
  __syncthreads();
  s = 0.0;
  for (int i = 0; i < nc; ++i) s += pc[(size_t)i * kLossBlocks + threadIdx.x];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) loss[1] = accumulate ? loss[1] + s : s;
}

// ---------------------------------------------------------------- Adam
__global__ void k_adam(int64_t n, float* w, const float* g, float* m, float* v, double lr, double b1, double b2,
                       double eps, double c1, double c2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double gi = g[i];
  const float mn = (float)(b1 * (double)m[i] + (1.0 - b1) * gi);
  const float vn = (float)(b2 * (double)v[i] + (1.0 - b2) * gi * gi);
  m[i] = mn;
  v[i] = vn;
  w[i] = (float)((double)w[i] - lr * ((double)mn / c1) / (sqrt((double)vn / c2) + eps));
}

// ---------------------------------------------------------------- the plan: shapes, weight offsets, workspace
struct SepActs { float *D1, *X2, *D2, *X3, *D3; };
struct SepIdx { int cin; size_t dw[3], pw[3], b[3]; };   // element offsets into weights / grad
struct DenseIdx { size_t w, b; };

struct Plan {
  int B, U, F, FT, A2, P, H, M, C0, I, R, PC, S;
  int hb[kMaxHeads];
  SepIdx init[kMaxInit], upd[kMaxIt];
  DenseIdx agg[kMaxIt][2], llr[kMaxHeads][2], chest[2];
  size_t num_weights;
  // workspace
  float *ns, *z0, *out56, *GA, *GB, *G56, *G64, *dS, *slab;
  SepActs ainit[kMaxInit], aupd[kMaxIt];
  float* state[kMaxIt + 1];
  float *ahid[kMaxIt], *asp[kMaxIt], *zcat[kMaxIt];
  struct Readout { float *hid[kMaxHeads], *llr[kMaxHeads], *dllr[kMaxHeads], *chid, *href, *dh; } ro[kMaxIt];
  double *part_d, *part_c;
  size_t bytes;
};

void make_plan(const nrx_desc& d, const nrx_train_io& io, void* base, Plan* pl) {
  Plan& p = *pl;
  p.B = io.shape.batch, p.U = io.shape.num_tx, p.F = io.shape.num_subcarriers, p.FT = p.F * kT;
  p.A2 = 2 * d.num_rx_ant, p.P = p.B * p.U * p.FT, p.H = num_heads(&d), p.M = d.num_mcs;
  p.C0 = (d.use_h_hat ? 2 : 1) * p.A2 + 2, p.I = io.num_it, p.R = io.multiloss ? io.num_it : 1;
  p.PC = ((p.P + kMaxSlabs - 1) / kMaxSlabs + 31) / 32 * 32;
  p.S = (p.P + p.PC - 1) / p.PC;
  for (int h = 0; h < p.H; ++h) p.hb[h] = head_bits(&d, h);
  // weight offsets, Keras order (nrx_model.cpp)
  size_t o = 0;
  auto sep = [&](SepIdx& s, int cin) {
    s.cin = cin;
    const int ci[3] = {cin, kHID, kHID}, co[3] = {kHID, kHID, kDS};
    for (int l = 0; l < 3; ++l) {
      s.dw[l] = o, o += 9 * (size_t)ci[l];
      s.pw[l] = o, o += (size_t)ci[l] * co[l];
      s.b[l] = o, o += co[l];
    }
  };
  auto den = [&](DenseIdx& x, int cin, int cout) {
    x.w = o, o += (size_t)cin * cout;
    x.b = o, o += cout;
  };
  for (int m = 0; m < p.H; ++m) sep(p.init[m], p.C0);
  for (int i = 0; i < d.num_it; ++i) {
    den(p.agg[i][0], kDS, kAGG);
    den(p.agg[i][1], kAGG, kDS);
    sep(p.upd[i], 2 * kDS + 2);
  }
  for (int h = 0; h < p.H; ++h) {
    den(p.llr[h][0], kDS, kHID);
    den(p.llr[h][1], kHID, p.hb[h]);
  }
  den(p.chest[0], kDS, kHID);
  den(p.chest[1], kHID, p.A2);
  p.num_weights = o;
  // workspace
  Carver ws(base);
  auto act = [&](int c) { return ws.take<float>((size_t)p.P * c); };
  auto sep_acts = [&](SepActs& a, int cin) {
    a.D1 = act(cin), a.X2 = act(kHID), a.D2 = act(kHID), a.X3 = act(kHID), a.D3 = act(kHID);
  };
  p.ns = ws.take<float>(p.B);
  p.z0 = act(p.C0);
  for (int m = 0; m < p.H; ++m) sep_acts(p.ainit[m], p.C0);
  for (int i = 0; i <= p.I; ++i) p.state[i] = act(kDS);
  for (int i = 0; i < p.I; ++i) {
    p.ahid[i] = act(kAGG), p.asp[i] = act(kDS), p.zcat[i] = act(2 * kDS + 2);
    sep_acts(p.aupd[i], 2 * kDS + 2);
  }
  for (int r = 0; r < p.R; ++r) {
    for (int h = 0; h < p.H; ++h) p.ro[r].hid[h] = act(kHID), p.ro[r].llr[h] = act(p.hb[h]), p.ro[r].dllr[h] = act(p.hb[h]);
    p.ro[r].chid = act(kHID), p.ro[r].href = act(p.A2), p.ro[r].dh = act(p.A2);
  }
  p.GA = act(kHID), p.GB = act(kHID), p.G56 = act(kDS), p.out56 = act(kDS), p.G64 = act(kAGG), p.dS = act(kDS);
  p.slab = ws.take<float>((size_t)p.S * (kHID + 1) * kHID);
  p.part_d = ws.take<double>((size_t)p.R * p.H * kLossBlocks);
  p.part_c = ws.take<double>((size_t)p.R * kLossBlocks);
  p.bytes = ws.bytes();
}

// ---------------------------------------------------------------- launch helpers
struct Run {
  const Plan& p;
  const nrx_train_io& io;
  hipStream_t st;
  hipError_t err = hipSuccess;

  bool ok() {
    if (err == hipSuccess) err = hipGetLastError();
    return err == hipSuccess;
  }
  static unsigned blocks(size_t n) { return (unsigned)((n + kTB - 1) / kTB); }
  const float* W(size_t o) const { return io.weights + o; }
  float* G(size_t o) const { return io.grad + o; }

  // Y = X W + b (+ res) (relu); W [K][N] row-major
  void fwd(const float* X, int K, size_t w, size_t b, int N, float* Y, bool relu, const float* res = nullptr) {
    if (!ok()) return;
    GemmArgs g{X, K, W(w), N, 1, W(b), res, N, nullptr, 0, Y, N, p.P, K, N, relu, 0};
    k_gemm<<<(p.P + 127) / 128, kTB, 0, st>>>(g);
  }
  // dX [P][K] (ldx) (+)= dZ [P][N] W^T, zeroed where mask <= 0
  void bwd_data(const float* dZ, int ldz, int N, size_t w, int K, float* dX, int ldx, const float* mask, int ldm,
                bool accumulate) {
    if (!ok()) return;
    GemmArgs g{dZ, ldz, W(w), 1, N, nullptr, nullptr, 0, mask, ldm, dX, ldx, p.P, N, K, 0, accumulate};
    k_gemm<<<(p.P + 127) / 128, kTB, 0, st>>>(g);
  }
  // grad[w .. w + (K + 1) N) += [X^T dZ ; column sums of dZ] (the bias follows its kernel in the weight list)
  void wgrad(const float* X, int ldx, int K, const float* dZ, int ldz, int N, size_t w) {
    if (!ok()) return;
    WgradArgs g{X, ldx, dZ, ldz, p.slab, p.P, K, N, p.PC};
    k_wgrad<<<p.S, kTB, 0, st>>>(g);
    const int n = (K + 1) * N;
    k_slab_sum<<<blocks(n), kTB, 0, st>>>(p.slab, p.S, n, G(w));
  }
  void dw_fwd(const float* x, int C, size_t w, float* out) {
    if (!ok()) return;
    k_dw<false><<<blocks((size_t)p.P * C), kTB, 0, st>>>(x, C, W(w), C, out, C, nullptr, 0, p.F, p.P);
  }
  void dw_bwd(const float* dD, int ldd, int C, size_t w, float* out, int ldo, const float* mask) {
    if (!ok()) return;
    k_dw<true><<<blocks((size_t)p.P * C), kTB, 0, st>>>(dD, ldd, W(w), C, out, ldo, mask, C, p.F, p.P);
  }
  void dw_grad(const float* x, int C, const float* dD, int ldd, size_t w) {
    if (!ok()) return;
    k_dwgrad<<<p.S, 128, 0, st>>>(x, C, dD, ldd, C, p.F, p.P, p.PC, p.slab);
    k_slab_sum<<<blocks(9 * C), kTB, 0, st>>>(p.slab, p.S, 9 * C, G(w));
  }

  // three separable convolutions on x [P][cin]; out [P][56] (+ res)
  void sep_fwd(const SepIdx& s, const SepActs& a, const float* x, float* out, const float* res) {
    dw_fwd(x, s.cin, s.dw[0], a.D1);
    fwd(a.D1, s.cin, s.pw[0], s.b[0], kHID, a.X2, true);
    dw_fwd(a.X2, kHID, s.dw[1], a.D2);
    fwd(a.D2, kHID, s.pw[1], s.b[1], kHID, a.X3, true);
    dw_fwd(a.X3, kHID, s.dw[2], a.D3);
    fwd(a.D3, kHID, s.pw[2], s.b[2], kDS, out, false, res);
  }
  // its backward from dOut [P][56]; with input_grad the gradient of x is left in GB (row stride 128)
  void sep_bwd(const SepIdx& s, const SepActs& a, const float* x, const float* dOut, bool input_grad) {
    wgrad(a.D3, kHID, kHID, dOut, kDS, kDS, s.pw[2]);
    bwd_data(dOut, kDS, kDS, s.pw[2], kHID, p.GA, kHID, nullptr, 0, false);
    dw_grad(a.X3, kHID, p.GA, kHID, s.dw[2]);
    dw_bwd(p.GA, kHID, kHID, s.dw[2], p.GB, kHID, a.X3);
    wgrad(a.D2, kHID, kHID, p.GB, kHID, kHID, s.pw[1]);
    bwd_data(p.GB, kHID, kHID, s.pw[1], kHID, p.GA, kHID, nullptr, 0, false);
    dw_grad(a.X2, kHID, p.GA, kHID, s.dw[1]);
    dw_bwd(p.GA, kHID, kHID, s.dw[1], p.GB, kHID, a.X2);
    wgrad(a.D1, s.cin, s.cin, p.GB, kHID, kHID, s.pw[0]);
    bwd_data(p.GB, kHID, kHID, s.pw[0], s.cin, p.GA, kHID, nullptr, 0, false);
    dw_grad(x, s.cin, p.GA, kHID, s.dw[0]);
    if (input_grad) dw_bwd(p.GA, kHID, s.cin, s.dw[0], p.GB, kHID, nullptr);
  }

  void readout_fwd(int r, const float* s) {
    const Plan::Readout& ro = p.ro[r];
    for (int h = 0; h < p.H; ++h) {
      fwd(s, kDS, p.llr[h][0].w, p.llr[h][0].b, kHID, ro.hid[h], true);
      fwd(ro.hid[h], kHID, p.llr[h][1].w, p.llr[h][1].b, p.hb[h], ro.llr[h], false);
    }
    fwd(s, kDS, p.chest[0].w, p.chest[0].b, kHID, ro.chid, true);
    fwd(ro.chid, kHID, p.chest[1].w, p.chest[1].b, p.A2, ro.href, false);
  }
  void dense2_bwd(const DenseIdx* L, const float* s, const float* hid, const float* dout, int nout, bool* first) {
    wgrad(hid, kHID, kHID, dout, nout, nout, L[1].w);
    bwd_data(dout, nout, nout, L[1].w, kHID, p.GA, kHID, hid, kHID, false);
    wgrad(s, kDS, kDS, p.GA, kHID, kHID, L[0].w);
    bwd_data(p.GA, kHID, kHID, L[0].w, kDS, p.dS, kDS, nullptr, 0, !*first);
    *first = false;
  }
  // the readout's backward into dS: overwritten by the first product when `first`, else added to
  void readout_bwd(int r, const float* s, bool first, bool chest) {
    const Plan::Readout& ro = p.ro[r];
    for (int h = 0; h < p.H; ++h) dense2_bwd(p.llr[h], s, ro.hid[h], ro.dllr[h], p.hb[h], &first);
    if (chest) dense2_bwd(p.chest, s, ro.chid, ro.dh, p.A2, &first);
  }
};

}  // namespace

size_t train_workspace_bytes(const nrx_desc& d, const nrx_train_io& io) {
  Plan p;
  make_plan(d, io, nullptr, &p);
  return p.bytes;
}

// The loss denominators carry batch_total, the B of the whole step, in place of this call's B: every term of a
// micro-batch then has the weight it has in the whole batch, and the sum over the calls is the step's loss and
// gradient with nothing to rescale.  An accumulating call skips the memset and adds its loss in f64; the slab
// sums add onto grad in their fixed order either way.
hipError_t launch_train_grad(const nrx_desc& d, const nrx_train_io& io, bool accumulate, int batch_total, void* ws,
                             hipStream_t st) {
  Plan p;
  make_plan(d, io, ws, &p);
  Run run{p, io, st};
  const int P = p.P;
  if (!accumulate) run.err = hipMemsetAsync(io.grad, 0, p.num_weights * sizeof(float), st);
  if (!run.ok()) return run.err;

  // ---- forward
  k_norm<<<p.B, kTB, 0, st>>>(io.y, p.FT * p.A2, p.ns);
  k_z0<<<Run::blocks((size_t)P * p.C0), kTB, 0, st>>>(io.y, io.pe, io.h_hat, p.ns, p.U, p.F, p.A2, p.C0, P, p.z0);
  for (int m = 0; m < p.H; ++m) {
    if (d.var_mcs_masking) {
      run.sep_fwd(p.init[m], p.ainit[m], p.z0, p.state[0], nullptr);
    } else {
      run.sep_fwd(p.init[m], p.ainit[m], p.z0, p.out56, nullptr);
      if (run.ok())
        k_rowscale<<<Run::blocks((size_t)P * kDS), kTB, 0, st>>>(p.out56, io.mcs_mask, p.M, m, p.FT, kDS, P, m > 0,
                                                                 p.state[0]);
    }
  }
  const int n_data = kT - __builtin_popcount(io.dmrs_symbol_mask);
  int nd = 0, nc = 0;
  auto readout = [&](int r, const float* s) {
    run.readout_fwd(r, s);
    if (!run.ok()) return;
    for (int h = 0; h < p.H; ++h) {
      LossLlrArgs g{};
      g.llr = p.ro[r].llr[h], g.bits = io.bits, g.bits_stride = io.bits_stride, g.active = io.active;
      g.mask = io.mcs_mask, g.M = p.M;
      g.m_lo = d.var_mcs_masking ? 0 : h, g.m_hi = d.var_mcs_masking ? p.M : h + 1;
      for (int m = 0; m < p.M; ++m) {
        g.bits_m[m] = d.bits[m];
        g.inv_den[m] = 1.0 / ((double)batch_total * p.U * p.F * n_data * d.bits[m]);
      }
      g.dmrs_mask = io.dmrs_symbol_mask, g.hb = p.hb[h], g.FT = p.FT, g.P = P;
      g.dllr = p.ro[r].dllr[h], g.part = p.part_d + (size_t)nd++ * kLossBlocks;
      k_loss_llr<<<kLossBlocks, kTB, 0, st>>>(g);
    }
    if (io.h)
      k_loss_chest<<<kLossBlocks, kTB, 0, st>>>(p.ro[r].href, io.h, io.active, p.FT, p.A2, P,
                                                1.0 / ((double)batch_total * p.U * p.FT * p.A2), io.w_chest,
                                                p.ro[r].dh,
                                                p.part_c + (size_t)nc++ * kLossBlocks);
  };
  for (int i = 0; i < p.I; ++i) {
    run.fwd(p.state[i], kDS, p.agg[i][0].w, p.agg[i][0].b, kAGG, p.ahid[i], true);
    run.fwd(p.ahid[i], kAGG, p.agg[i][1].w, p.agg[i][1].b, kDS, p.asp[i], false);
    if (run.ok())
      k_concat<<<Run::blocks((size_t)P * (2 * kDS + 2)), kTB, 0, st>>>(p.asp[i], p.state[i], io.pe, io.active, p.U,
                                                                       p.F, P, p.zcat[i]);
    run.sep_fwd(p.upd[i], p.aupd[i], p.zcat[i], p.state[i + 1], p.state[i]);
    if (io.multiloss || i == p.I - 1) readout(io.multiloss ? i : 0, p.state[i + 1]);
  }
  if (!run.ok()) return run.err;
  k_loss_sum<<<1, kTB, 0, st>>>(p.part_d, nd, p.part_c, nc, accumulate, io.loss);
  const Plan::Readout& last = p.ro[p.R - 1];
  if (io.llr) {
    const int bm = bits_max(&d);
    for (int h = 0; h < p.H; ++h)
      k_copy_cols<<<Run::blocks((size_t)P * bm), kTB, 0, st>>>(last.llr[h], p.hb[h], io.llr + (size_t)h * P * bm, bm, P);
  }
  if (io.h_ref)
    k_copy_cols<<<Run::blocks((size_t)P * p.A2), kTB, 0, st>>>(last.href, p.A2, io.h_ref, p.A2, P);

  // ---- backward: dS holds the gradient of the state the loop stands at
  const bool chest = io.h && io.w_chest > 0.0;
  run.readout_bwd(p.R - 1, p.state[p.I], /*first=*/true, chest);
  for (int i = p.I - 1; i >= 0; --i) {
    run.sep_bwd(p.upd[i], p.aupd[i], p.zcat[i], p.dS, /*input_grad=*/true);
    if (run.ok())
      k_concat_bwd<<<Run::blocks((size_t)P * kDS), kTB, 0, st>>>(p.GB, kHID, io.active, p.U, p.F, P, p.dS, p.G56);
    run.wgrad(p.ahid[i], kAGG, kAGG, p.G56, kDS, kDS, p.agg[i][1].w);
    run.bwd_data(p.G56, kDS, kDS, p.agg[i][1].w, kAGG, p.G64, kAGG, p.ahid[i], kAGG, false);
    run.wgrad(p.state[i], kDS, kDS, p.G64, kAGG, kAGG, p.agg[i][0].w);
    run.bwd_data(p.G64, kAGG, kAGG, p.agg[i][0].w, kDS, p.dS, kDS, nullptr, 0, true);
    if (io.multiloss && i >= 1) run.readout_bwd(i - 1, p.state[i], /*first=*/false, chest);
  }
  for (int m = 0; m < p.H; ++m) {
    const float* dOut = p.dS;
    if (!d.var_mcs_masking) {
      if (run.ok())
        k_rowscale<<<Run::blocks((size_t)P * kDS), kTB, 0, st>>>(p.dS, io.mcs_mask, p.M, m, p.FT, kDS, P, 0, p.G56);
      dOut = p.G56;
    }
    run.sep_bwd(p.init[m], p.ainit[m], p.z0, dOut, /*input_grad=*/false);
  }
  run.ok();
  return run.err;
}

hipError_t launch_adam(const nrx_adam_io& io, double c1, double c2, hipStream_t st) {
  if (io.n == 0) return hipSuccess;
  k_adam<<<(unsigned)((io.n + kTB - 1) / kTB), kTB, 0, st>>>(io.n, io.w, io.g, io.m, io.v, io.lr, io.beta1, io.beta2,
                                                            io.eps, c1, c2);
  return hipGetLastError();
}

}  // namespace nrx
