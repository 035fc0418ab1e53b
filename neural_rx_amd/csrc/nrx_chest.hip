// nrx_chest.hip -- channel-estimation baselines on the GPU (include/nrx.h): the covariance lag
// sums of the generator's channel (nrx_cov_accumulate), the 2-D LMMSE (Wiener) estimator
// (nrx_chest_lmmse) and the linear interpolator (nrx_chest_lin) -- the estimators of the reference's
// baseline_lmmse_lmmse / baseline_lslin_lmmse systems (utils/baseline_rx.py:100-229) and of its
// scripts/compute_cov_mat.py.
//
// nrx_chest_lmmse.  Per (slot b, user u) the estimate is h^[f, t] = sum_k a_k[t] (W_k z_k)[f] with
// z_k = sum_d conj(v_k[d]) h_ls[P, D_d] (host design: neural_rx_amd/chest.py).  Y_k = W_k z_k is a
// complex F x |P| by |P| x A product; with the K axis ordered (pilot, re / im) it is two real GEMMs
// that share their A operand, the filter table as it lies in memory:
//   Re Y = [Wr Wi] . [zr; -zi],   Im Y = [Wr Wi] . [zi; zr]            (K = 2 |P|, N = A <= 16)
// on the exact-f32 MFMA v_mfma_f32_16x16x4_f32: in step (S, j) lane l holds W[row l & 15] of pilot
// 16 S + 4 (l >> 4) + j as one 8-byte load (re = K step 0, im = K step 1) and reads zr / zi of that
// pilot and antenna l & 15 from LDS.  A workgroup is 4 waves = 4 tiles of 16 subcarriers of one (b, u); z is staged
// in chunks of 32 pilots.  The 14-symbol expansion by a_k[t] is the epilogue: the Y tiles go
// through LDS so that every wave writes its 16 x 14 x 2A output floats as one contiguous run.
// f32 throughout, no atomics: outputs are deterministic and do not depend on the batch split.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nrx.h"
#include "nrx_internal.h"

namespace nrx {

namespace {

// ------------------------------------------------------------------ covariance lag sums
constexpr int kCovBlock = 256;
constexpr int kCovGroups = 256;     // partial sums per lag (fixed: the sum order is part of the result)
constexpr int kMaxF = 3300;

struct CovArgs {
  int F, A, groups;
  int64_t rows_f;       // B * U * T * A rows of F subcarriers
  int64_t cols_t;       // B * U * F * A columns of T symbols
  const float* h;
  double* part;         // [groups][F + 14][2]
  double* acc;          // [F + 14][2]
};

// Workgroup g sums its rows' frequency lags (a row of F complex values staged in LDS, lane = lag)
// and its columns' time lags (14 values in registers, fixed-order wave + workgroup reduction) into
// its own slice of `part`; f64 products and sums.
__global__ __launch_bounds__(kCovBlock) void k_cov_partial(CovArgs p) {
  __shared__ float2 row[kMaxF];
  __shared__ double red[kCovBlock / 64][2 * kT];
  const int tid = threadIdx.x, g = blockIdx.x;
  const int F = p.F, A = p.A;
  double* part = p.part + (size_t)g * (F + kT) * 2;
  for (int d = tid; d < F; d += kCovBlock) part[2 * d] = part[2 * d + 1] = 0.0;
  for (int64_t r = g; r < p.rows_f; r += p.groups) {
    const int a = (int)(r % A);
    const int t = (int)((r / A) % kT);
    const int64_t bu = r / ((int64_t)A * kT);
    const float* src = p.h + ((size_t)bu * F * kT + t) * 2 * A + a;
    __syncthreads();                                   // the previous row has been read
    for (int f = tid; f < F; f += kCovBlock)
      row[f] = make_float2(src[(size_t)f * kT * 2 * A], src[(size_t)f * kT * 2 * A + A]);
    __syncthreads();
    for (int d = tid; d < F; d += kCovBlock) {         // the lane owns lag d and its slot of part
      double sr = 0.0, si = 0.0;
      for (int f = 0; f + d < F; ++f) {
        const float2 x = row[f + d], y = row[f];       // x conj(y)
        sr += (double)x.x * (double)y.x + (double)x.y * (double)y.y;
        si += (double)x.y * (double)y.x - (double)x.x * (double)y.y;
      }
      part[2 * d] += sr;
      part[2 * d + 1] += si;
    }
  }
  double tr[kT], ti[kT];
#pragma unroll
  for (int d = 0; d < kT; ++d) tr[d] = ti[d] = 0.0;
  for (int64_t c = (int64_t)g * kCovBlock + tid; c < p.cols_t; c += (int64_t)p.groups * kCovBlock) {
    const int a = (int)(c % A);
    const int f = (int)((c / A) % F);
    const int64_t bu = c / ((int64_t)A * F);
    const float* src = p.h + ((size_t)bu * F + f) * kT * 2 * A + a;
    double xr[kT], xi[kT];
#pragma unroll
    for (int t = 0; t < kT; ++t) {
      xr[t] = (double)src[t * 2 * A];
      xi[t] = (double)src[t * 2 * A + A];
    }
#pragma unroll
    for (int d = 0; d < kT; ++d) {
#pragma unroll
      for (int t = 0; t + d < kT; ++t) {
        tr[d] += xr[t + d] * xr[t] + xi[t + d] * xi[t];
        ti[d] += xi[t + d] * xr[t] - xr[t + d] * xi[t];
      }
    }
  }
#pragma unroll
  for (int d = 0; d < kT; ++d) {
    double vr = tr[d], vi = ti[d];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      vr += __shfl_down(vr, off);
      vi += __shfl_down(vi, off);
    }
    if ((tid & 63) == 0) {
      red[tid >> 6][2 * d] = vr;
      red[tid >> 6][2 * d + 1] = vi;
    }
  }
  __syncthreads();
  if (tid < 2 * kT) part[2 * F + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// acc[i] += sum_g part[g][i], g ascending: one lane per output, no atomics
__global__ __launch_bounds__(kCovBlock) void k_cov_reduce(CovArgs p) {
  const int n = (p.F + kT) * 2;
  const int i = blockIdx.x * kCovBlock + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int g = 0; g < p.groups; ++g) s += p.part[(size_t)g * n + i];
  p.acc[i] += s;
}

int cov_groups(const nrx_cov_io& io) {
  const int64_t rows = (int64_t)io.batch * io.num_tx * kT * io.num_rx_ant;
  return (int)(rows < kCovGroups ? rows : kCovGroups);
}

// ------------------------------------------------------------------ spatial covariance sums
struct CovSpaceArgs {
  int A, groups;
  int64_t rows;         // B * U * F * T resource elements of 2A floats
  const float* h;
  double* part;         // [groups][A * A][2]
  double* acc;          // [A * A][2]
};

// Thread (s, p) of workgroup g owns the antenna pair p = (a, a') and walks the resource elements
// r = g * S + s, + groups * S, ... (S = 256 / A^2 walkers per pair): the lanes of a pair group read
// one 2A-float row together, so every row comes from HBM once.  The S walkers of a pair are summed
// in ascending s by the pair's first thread: a fixed order, f64 throughout.
__global__ __launch_bounds__(kCovBlock) void k_cov_space_partial(CovSpaceArgs p) {
  __shared__ double red[kCovBlock][2];
  const int tid = threadIdx.x, g = blockIdx.x;
  const int A = p.A, AA = A * A, S = kCovBlock / AA;
  const int s = tid / AA, pr = tid - s * AA;
  const int a = pr / A, a2 = pr - a * A;
  double sr = 0.0, si = 0.0;
  if (s < S) {
    for (int64_t r = (int64_t)g * S + s; r < p.rows; r += (int64_t)p.groups * S) {
      const float* src = p.h + (size_t)r * 2 * A;
      const double xr = src[a], xi = src[A + a], yr = src[a2], yi = src[A + a2];   // x conj(y)
      sr += xr * yr + xi * yi;
      si += xi * yr - xr * yi;
    }
  }
  red[tid][0] = sr;
  red[tid][1] = si;
  __syncthreads();
  if (tid < AA) {
    double tr = 0.0, ti = 0.0;
    for (int k = 0; k < S; ++k) {
      tr += red[k * AA + tid][0];
      ti += red[k * AA + tid][1];
    }
    p.part[((size_t)g * AA + tid) * 2] = tr;
    p.part[((size_t)g * AA + tid) * 2 + 1] = ti;
  }
}

// acc[i] += sum_g part[g][i], g ascending: one lane per output, no atomics
__global__ __launch_bounds__(kCovBlock) void k_cov_space_reduce(CovSpaceArgs p) {
  const int n = p.A * p.A * 2;
  const int i = blockIdx.x * kCovBlock + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int g = 0; g < p.groups; ++g) s += p.part[(size_t)g * n + i];
  p.acc[i] += s;
}

int cov_space_groups(const nrx_cov_space_io& io) {
  const int64_t rows = (int64_t)io.batch * io.num_tx * io.num_subcarriers * kT;
  return (int)(rows < kCovGroups ? rows : kCovGroups);
}

// ------------------------------------------------------------------ the estimators
constexpr int kChBlock = 256;
constexpr int kChWaves = kChBlock / 64;
constexpr int kPC = 32;             // pilots per staged chunk of z
constexpr int kZG = 80;             // floats per group of 4 pilots in the z image: 4 x 16 antennas + 16 of
                                    // padding, so that the lanes' pilots 4 (l >> 4) + j fall into distinct banks
__device__ __forceinline__ int z_at(int pp, int a) { return (pp >> 2) * kZG + (pp & 3) * 16 + a; }

struct ChestArgs {
  int B, U, F, A, nd;
  int dm[4];
  unsigned grp_mask;                // bit u: cdm_group[u]
  const float* hh;
  const float* active;
  const float* filt;                // [2][nd][F][Pmax][2]
  const float* tcoef;               // [nd][14][2]
  const float* vconj;               // [nd][nd][2]
  float* out;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int ND, bool VEC>
__global__ __launch_bounds__(kChBlock) void k_chest_lmmse(ChestArgs p) {
  __shared__ float zs[ND][2][kPC / 4 * kZG];        // z_k chunk [k][re / im][z_at(pilot, antenna)]
  __shared__ float ys[kChWaves][ND][2][16][16];     // per wave: Y_k tile [k][re / im][row][antenna]
  __shared__ float tc[ND * kT * 2];
  __shared__ float vc[ND * ND * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // blockIdx.x = (b, u), the fast axis of the dispatch order: the workgroups in flight share a few
  // tile rows of the filter table, which then stays in L2 across the batch
  const int bu = blockIdx.x, u = bu % p.U;
  const int F = p.F, A = p.A, A2 = 2 * A;
  const int f0 = (blockIdx.y * kChWaves + wave) * 16;
  const int nrow = F - f0 < 16 ? F - f0 : 16;       // <= 0: no tile for this wave
  const int n = nrow * kT * A2;                     // this wave's output floats, one contiguous run
  float* dst = p.out + ((size_t)bu * F + (nrow > 0 ? f0 : 0)) * kT * A2;
  if (!(p.active[bu] > 0.0f)) {                     // uniform over the workgroup
    if (VEC) {
      for (int e = lane * 4; e < n; e += 256) *reinterpret_cast<float4*>(dst + e) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int e = lane; e < n; e += 64) dst[e] = 0.0f;
    }
    return;
  }
  const int g = (p.grp_mask >> u) & 1;
  const int P = (F - g + 1) >> 1;                   // own pilots: f = g, g + 2, ...
  const int Pmax = (F + 1) >> 1;
  if (tid < ND * kT * 2) tc[tid] = p.tcoef[tid];
  if (tid < ND * ND * 2) vc[tid] = p.vconj[tid];
  f32x4 accr[ND], acci[ND];
#pragma unroll
  for (int k = 0; k < ND; ++k) accr[k] = acci[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int col = lane & 15, kk = lane >> 4;
  const int frow = f0 + col < F ? f0 + col : F - 1; // rows past F are computed on row F - 1 and dropped
  const float* hb = p.hh + (size_t)bu * F * kT * A2;
  const float2* wrow[ND];
#pragma unroll
  for (int k = 0; k < ND; ++k)
    wrow[k] = reinterpret_cast<const float2*>(p.filt) + ((size_t)(g * ND + k) * F + frow) * Pmax;

  for (int pc = 0; pc < P; pc += kPC) {
    // this chunk's A operand, issued ahead of the staging so that its latency hides behind it: lane
    // (row, kk) takes pilots 16 S + 4 kk + j, j < 4 -- 32 contiguous bytes, and the four kk lanes of
    // a row one whole 128-byte line at a time
    float2 wv[ND][kPC / 4];
#pragma unroll
    for (int i = 0; i < kPC / 4; ++i) {
      const int pp = pc + 16 * (i >> 2) + 4 * kk + (i & 3);
#pragma unroll
      for (int k = 0; k < ND; ++k) wv[k][i] = nrow > 0 && pp < P ? wrow[k][pp] : make_float2(0.f, 0.f);
    }
    __syncthreads();                                // vc is there; the previous chunk has been read
    for (int e = tid; e < kPC * 16; e += kChBlock) {
      const int pp = e >> 4, a = e & 15;
      float zr[ND], zi[ND];
#pragma unroll
      for (int k = 0; k < ND; ++k) zr[k] = zi[k] = 0.0f;
      if (pc + pp < P && a < A) {
        const float* src = hb + (size_t)(g + 2 * (pc + pp)) * kT * A2 + a;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          const float xr = src[p.dm[d] * A2], xi = src[p.dm[d] * A2 + A];
#pragma unroll
          for (int k = 0; k < ND; ++k) {
            const float cr = vc[(k * ND + d) * 2], ci = vc[(k * ND + d) * 2 + 1];
            zr[k] += cr * xr - ci * xi;
            zi[k] += cr * xi + ci * xr;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        zs[k][0][z_at(pp, a)] = zr[k];
        zs[k][1][z_at(pp, a)] = zi[k];
      }
    }
    __syncthreads();
    if (nrow > 0) {
#pragma unroll
      for (int i = 0; i < kPC / 4; ++i) {
        if (pc + 16 * (i >> 2) < P) {               // uniform
          const int pp = 16 * (i >> 2) + 4 * kk + (i & 3);
#pragma unroll
          for (int k = 0; k < ND; ++k) {
            const float2 w = wv[k][i];
            const float zr = zs[k][0][z_at(pp, col)], zi = zs[k][1][z_at(pp, col)];
            accr[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, zr, accr[k], 0, 0, 0);
            acci[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, zi, acci[k], 0, 0, 0);
            accr[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, -zi, accr[k], 0, 0, 0);
            acci[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, zr, acci[k], 0, 0, 0);
          }
        }
      }
    }
  }
  // C / D layout: column = lane & 15 (antenna), row = 4 (lane >> 4) + register (subcarrier)
#pragma unroll
  for (int k = 0; k < ND; ++k) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ys[wave][k][0][kk * 4 + r][col] = accr[k][r];
      ys[wave][k][1][kk * 4 + r][col] = acci[k][r];
    }
  }
  __syncthreads();
  const int rowlen = kT * A2;
  if (VEC) {
    for (int e = lane * 4; e < n; e += 256) {
      const int fr = e / rowlen, rem = e - fr * rowlen;
      const int t = rem / A2, c = rem - t * A2;
      const bool im = c >= A;
      const int a = im ? c - A : c;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        const float ar = tc[(k * kT + t) * 2], ai = tc[(k * kT + t) * 2 + 1];
        const float4 yr = *reinterpret_cast<const float4*>(&ys[wave][k][0][fr][a]);
        const float4 yi = *reinterpret_cast<const float4*>(&ys[wave][k][1][fr][a]);
        const float c0 = im ? ai : ar, c1 = im ? ar : -ai;       // re: ar yr - ai yi, im: ai yr + ar yi
        o.x += c0 * yr.x + c1 * yi.x;
        o.y += c0 * yr.y + c1 * yi.y;
        o.z += c0 * yr.z + c1 * yi.z;
        o.w += c0 * yr.w + c1 * yi.w;
      }
      *reinterpret_cast<float4*>(dst + e) = o;
    }
  } else {
    for (int e = lane; e < n; e += 64) {
      const int fr = e / rowlen, rem = e - fr * rowlen;
      const int t = rem / A2, c = rem - t * A2;
      const bool im = c >= A;
      const int a = im ? c - A : c;
      float o = 0.0f;
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        const float ar = tc[(k * kT + t) * 2], ai = tc[(k * kT + t) * 2 + 1];
        const float c0 = im ? ai : ar, c1 = im ? ar : -ai;
        o += c0 * ys[wave][k][0][fr][a] + c1 * ys[wave][k][1][fr][a];
      }
      dst[e] = o;
    }
  }
}

// One lane per 4 output floats (VEC; else per float) of a row (b, u, f, t), so that a wave's stores
// are one contiguous run.  Linear in frequency between the two own pilots that bracket f (the two
// nearest ones beyond the first / last pilot), then linear in time between the two DMRS symbols
// that bracket t; a single pilot or symbol is repeated.
template <bool VEC>
__global__ __launch_bounds__(kChBlock) void k_chest_lin(ChestArgs p, int64_t nvec) {
  constexpr int W = VEC ? 4 : 1;
  const int64_t iv = (int64_t)blockIdx.x * kChBlock + threadIdx.x;
  if (iv >= nvec) return;
  const int F = p.F, A2 = 2 * p.A;
  const int per_row = A2 / W;
  const int64_t i = iv / per_row;                   // row (b, u, f, t)
  const int c = (int)(iv - i * per_row) * W;
  const int FT = F * kT;
  const int64_t bu = i / FT;
  const int ft = (int)(i - bu * FT);
  const int f = ft / kT, t = ft - f * kT;
  float* dst = p.out + (size_t)i * A2 + c;
  const int g = (p.grp_mask >> (int)(bu % p.U)) & 1;
  const int P = (F - g + 1) >> 1;
  if (!(p.active[bu] > 0.0f) || P < 1) {
    if (VEC) *reinterpret_cast<float4*>(dst) = make_float4(0.f, 0.f, 0.f, 0.f);
    else *dst = 0.0f;
    return;
  }
  int p0 = g, p1 = g;
  float wf = 0.0f;
  if (P > 1) {
    int j = (f - g) / 2;
    j = j < 0 ? 0 : (j > P - 2 ? P - 2 : j);
    p0 = g + 2 * j;
    p1 = p0 + 2;
    wf = 0.5f * (float)(f - p0);
  }
  int t0 = p.dm[0], t1 = p.dm[0];
  float wt = 0.0f;
  if (p.nd > 1) {
    t1 = p.dm[1];
#pragma unroll
    for (int k = 1; k < 3; ++k) {
      if (k < p.nd - 1 && t >= p.dm[k]) {
        t0 = p.dm[k];
        t1 = p.dm[k + 1];
      }
    }
    wt = (float)(t - t0) / (float)(t1 - t0);
  }
  const float* hb = p.hh + (size_t)bu * FT * A2 + c;
  const float* s00 = hb + ((size_t)p0 * kT + t0) * A2;
  const float* s10 = hb + ((size_t)p1 * kT + t0) * A2;
  const float* s01 = hb + ((size_t)p0 * kT + t1) * A2;
  const float* s11 = hb + ((size_t)p1 * kT + t1) * A2;
  const float uf = 1.0f - wf, ut = 1.0f - wt;
#define NRX_LIN(x00, x10, x01, x11) (ut * (uf * (x00) + wf * (x10)) + wt * (uf * (x01) + wf * (x11)))
  if (VEC) {
    const float4 a = *reinterpret_cast<const float4*>(s00), b = *reinterpret_cast<const float4*>(s10);
    const float4 d = *reinterpret_cast<const float4*>(s01), e = *reinterpret_cast<const float4*>(s11);
    *reinterpret_cast<float4*>(dst) = make_float4(NRX_LIN(a.x, b.x, d.x, e.x), NRX_LIN(a.y, b.y, d.y, e.y),
                                                   NRX_LIN(a.z, b.z, d.z, e.z), NRX_LIN(a.w, b.w, d.w, e.w));
  } else {
    *dst = NRX_LIN(*s00, *s10, *s01, *s11);
  }
#undef NRX_LIN
}

// ------------------------------------------------------------------ the 3-D (space-time-frequency) filter
// nrx_chest_lmmse3 (include/nrx.h): the exact Wiener filter under R_s (x) R_t (x) R_f, diagonal in the
// three eigenbases.  Two launches around a workspace c' [B U][Pmax][nd][2A]:
//   k_chest3_pilot   w = Q_g^H . z on the MFMA (M = eigen-component q, K = pilot p, N = spatial
//                    component j), z = (V_s^H (x) V_t^H) h_ls applied while staging; then the gain
//                    mu_j / (mu_j lambda_k nu_q + sigma^2) and the rotation back to antennas
//                    c'[a] = sum_j V_s[a][j] c[j] in the epilogue.  The rotation commutes with the
//                    frequency product of the second stage, so it is done here, on |P| rows, and not
//                    there, on F rows.
//   k_chest3_expand  Y_k = G_g . c'_k on the MFMA (M = subcarrier, K = q, N = antenna) and the
//                    14-symbol expansion by tcoef: k_chest_lmmse with one A operand for all k.
// Both read the A operand (rows of qh / gf) once for all nd components.
struct Chest3Args {
  int B, U, F, A, nd;
  int dm[4];
  unsigned grp_mask;                // bit u: cdm_group[u]
  float sigma2;                     // no / 2
  const float* hh;
  const float* active;
  const float* qh;                  // [2][Pmax][Pmax][2]
  const float* gf;                  // [2][F][Pmax][2]
  const float* nu;                  // [2][Pmax]
  const float* tcoef;               // [nd][14][2]
  const float* vconj;               // [nd][nd][2]
  const float* lam;                 // [nd]
  const float* vs;                  // [A][A][2]
  const float* mu;                  // [A]
  float* cw;                        // [B U][Pmax][nd][2A]
  float* out;
};

template <int ND>
__global__ __launch_bounds__(kChBlock) void k_chest3_pilot(Chest3Args p) {
  __shared__ float zs[ND][2][kPC / 4 * kZG];        // z chunk [k][re / im][z_at(pilot, component j)]
  __shared__ float ys[kChWaves][ND][2][16][16];     // per wave: c tile [k][re / im][row q][component j]
  __shared__ float vc[ND * ND * 2];
  __shared__ float vsr[16 * 16], vsi[16 * 16];      // V_s[a][j] at [a * 16 + j], zero beyond A
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bu = blockIdx.x, u = bu % p.U;
  if (!(p.active[bu] > 0.0f)) return;               // uniform; k_chest3_expand writes the zeros and reads no c'
  const int F = p.F, A = p.A, A2 = 2 * A;
  const int g = (p.grp_mask >> u) & 1;
  const int P = (F - g + 1) >> 1;
  const int Pmax = (F + 1) >> 1;
  const int q0 = (blockIdx.y * kChWaves + wave) * 16;
  const int nrow = P - q0 < 16 ? P - q0 : 16;       // <= 0: no tile for this wave
  if (tid < ND * ND * 2) vc[tid] = p.vconj[tid];
  {
    const int a = tid >> 4, j = tid & 15;
    const bool ok = a < A && j < A;
    vsr[tid] = ok ? p.vs[(a * A + j) * 2] : 0.0f;
    vsi[tid] = ok ? p.vs[(a * A + j) * 2 + 1] : 0.0f;
  }
  f32x4 accr[ND], acci[ND];
#pragma unroll
  for (int k = 0; k < ND; ++k) accr[k] = acci[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int col = lane & 15, kk = lane >> 4;
  int qrow = q0 + col < P ? q0 + col : P - 1;       // rows past P are computed on row P - 1 and dropped
  qrow = qrow < 0 ? 0 : qrow;
  const float* hb = p.hh + (size_t)bu * F * kT * A2;
  const float2* wrow = reinterpret_cast<const float2*>(p.qh) + ((size_t)g * Pmax + qrow) * Pmax;

  for (int pc = 0; pc < P; pc += kPC) {
    float2 wv[kPC / 4];
#pragma unroll
    for (int i = 0; i < kPC / 4; ++i) {
      const int pp = pc + 16 * (i >> 2) + 4 * kk + (i & 3);
      wv[i] = nrow > 0 && pp < P ? wrow[pp] : make_float2(0.f, 0.f);
    }
    __syncthreads();                                // the tables are there; the previous chunk has been read
    for (int e = tid; e < kPC * 16; e += kChBlock) {
      const int pp = e >> 4, j = e & 15;
      float zr[ND], zi[ND];
#pragma unroll
      for (int k = 0; k < ND; ++k) zr[k] = zi[k] = 0.0f;
      if (pc + pp < P && j < A) {
        const float* src = hb + (size_t)(g + 2 * (pc + pp)) * kT * A2;
        for (int a = 0; a < A; ++a) {
          float yr[ND], yi[ND];
#pragma unroll
          for (int k = 0; k < ND; ++k) yr[k] = yi[k] = 0.0f;
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            const float xr = src[p.dm[d] * A2 + a], xi = src[p.dm[d] * A2 + A + a];
#pragma unroll
            for (int k = 0; k < ND; ++k) {
              const float cr = vc[(k * ND + d) * 2], ci = vc[(k * ND + d) * 2 + 1];
              yr[k] += cr * xr - ci * xi;
              yi[k] += cr * xi + ci * xr;
            }
          }
          const float sr = vsr[a * 16 + j], si = -vsi[a * 16 + j];      // conj(V_s[a][j])
#pragma unroll
          for (int k = 0; k < ND; ++k) {
            zr[k] += sr * yr[k] - si * yi[k];
            zi[k] += sr * yi[k] + si * yr[k];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        zs[k][0][z_at(pp, j)] = zr[k];
        zs[k][1][z_at(pp, j)] = zi[k];
      }
    }
    __syncthreads();
    if (nrow > 0) {
#pragma unroll
      for (int i = 0; i < kPC / 4; ++i) {
        if (pc + 16 * (i >> 2) < P) {               // uniform
          const int pp = 16 * (i >> 2) + 4 * kk + (i & 3);
          const float2 w = wv[i];
#pragma unroll
          for (int k = 0; k < ND; ++k) {
            const float zr = zs[k][0][z_at(pp, col)], zi = zs[k][1][z_at(pp, col)];
            accr[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, zr, accr[k], 0, 0, 0);
            acci[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, zi, acci[k], 0, 0, 0);
            accr[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, -zi, accr[k], 0, 0, 0);
            acci[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, zr, acci[k], 0, 0, 0);
          }
        }
      }
    }
  }
  // C / D layout: column = lane & 15 (component j), row = 4 (lane >> 4) + register (component q); the
  // gain is element-wise there
  const float muj = col < A ? p.mu[col] : 0.0f;
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    const float lk = p.lam[k];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + kk * 4 + r;
      const float nq = q < P ? p.nu[g * Pmax + q] : 0.0f;
      const float gain = muj / (muj * lk * nq + p.sigma2);
      ys[wave][k][0][kk * 4 + r][col] = accr[k][r] * gain;
      ys[wave][k][1][kk * 4 + r][col] = acci[k][r] * gain;
    }
  }
  __syncthreads();
  if (nrow <= 0) return;
  // back to antennas, c'[a] = sum_j V_s[a][j] c[j]; the wave's rows are one contiguous run of c'
  const int n = nrow * ND * A2;
  float* dst = p.cw + ((size_t)bu * Pmax + q0) * ND * A2;
  for (int e = lane; e < n; e += 64) {
    const int row = e / (ND * A2), rem = e - row * (ND * A2);
    const int k = rem / A2, c = rem - k * A2;
    const bool im = c >= A;
    const int a = im ? c - A : c;
    float o = 0.0f;
    for (int j = 0; j < A; ++j) {
      const float vr = vsr[a * 16 + j], vi = vsi[a * 16 + j];
      const float yr = ys[wave][k][0][row][j], yi = ys[wave][k][1][row][j];
      o += im ? vr * yi + vi * yr : vr * yr - vi * yi;
    }
    dst[e] = o;
  }
}

template <int ND, bool VEC>
__global__ __launch_bounds__(kChBlock) void k_chest3_expand(Chest3Args p) {
  __shared__ float zs[ND][2][kPC / 4 * kZG];        // c' chunk [k][re / im][z_at(component q, antenna)]
  __shared__ float ys[kChWaves][ND][2][16][16];     // per wave: Y_k tile [k][re / im][row][antenna]
  __shared__ float tc[ND * kT * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bu = blockIdx.x, u = bu % p.U;
  const int F = p.F, A = p.A, A2 = 2 * A;
  const int f0 = (blockIdx.y * kChWaves + wave) * 16;
  const int nrow = F - f0 < 16 ? F - f0 : 16;       // <= 0: no tile for this wave
  const int n = nrow * kT * A2;                     // this wave's output floats, one contiguous run
  float* dst = p.out + ((size_t)bu * F + (nrow > 0 ? f0 : 0)) * kT * A2;
  if (!(p.active[bu] > 0.0f)) {                     // uniform over the workgroup
    if (VEC) {
      for (int e = lane * 4; e < n; e += 256) *reinterpret_cast<float4*>(dst + e) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int e = lane; e < n; e += 64) dst[e] = 0.0f;
    }
    return;
  }
  const int g = (p.grp_mask >> u) & 1;
  const int P = (F - g + 1) >> 1;
  const int Pmax = (F + 1) >> 1;
  if (tid < ND * kT * 2) tc[tid] = p.tcoef[tid];
  f32x4 accr[ND], acci[ND];
#pragma unroll
  for (int k = 0; k < ND; ++k) accr[k] = acci[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int col = lane & 15, kk = lane >> 4;
  const int frow = f0 + col < F ? f0 + col : F - 1; // rows past F are computed on row F - 1 and dropped
  const float* cb = p.cw + (size_t)bu * Pmax * ND * A2;
  const float2* wrow = reinterpret_cast<const float2*>(p.gf) + ((size_t)g * F + frow) * Pmax;

  for (int pc = 0; pc < P; pc += kPC) {
    float2 wv[kPC / 4];
#pragma unroll
    for (int i = 0; i < kPC / 4; ++i) {
      const int pp = pc + 16 * (i >> 2) + 4 * kk + (i & 3);
      wv[i] = nrow > 0 && pp < P ? wrow[pp] : make_float2(0.f, 0.f);
    }
    __syncthreads();                                // the previous chunk has been read
    for (int e = tid; e < kPC * 16; e += kChBlock) {
      const int pp = e >> 4, a = e & 15;
      float zr[ND], zi[ND];
#pragma unroll
      for (int k = 0; k < ND; ++k) zr[k] = zi[k] = 0.0f;
      if (pc + pp < P && a < A) {
        const float* src = cb + (size_t)(pc + pp) * ND * A2 + a;
#pragma unroll
        for (int k = 0; k < ND; ++k) {
          zr[k] = src[k * A2];
          zi[k] = src[k * A2 + A];
        }
      }
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        zs[k][0][z_at(pp, a)] = zr[k];
        zs[k][1][z_at(pp, a)] = zi[k];
      }
    }
    __syncthreads();
    if (nrow > 0) {
#pragma unroll
      for (int i = 0; i < kPC / 4; ++i) {
        if (pc + 16 * (i >> 2) < P) {               // uniform
          const int pp = 16 * (i >> 2) + 4 * kk + (i & 3);
          const float2 w = wv[i];
#pragma unroll
          for (int k = 0; k < ND; ++k) {
            const float zr = zs[k][0][z_at(pp, col)], zi = zs[k][1][z_at(pp, col)];
            accr[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, zr, accr[k], 0, 0, 0);
            acci[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, zi, acci[k], 0, 0, 0);
            accr[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, -zi, accr[k], 0, 0, 0);
            acci[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, zr, acci[k], 0, 0, 0);
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < ND; ++k) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ys[wave][k][0][kk * 4 + r][col] = accr[k][r];
      ys[wave][k][1][kk * 4 + r][col] = acci[k][r];
    }
  }
  __syncthreads();
  const int rowlen = kT * A2;
  if (VEC) {
    for (int e = lane * 4; e < n; e += 256) {
      const int fr = e / rowlen, rem = e - fr * rowlen;
      const int t = rem / A2, c = rem - t * A2;
      const bool im = c >= A;
      const int a = im ? c - A : c;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        const float ar = tc[(k * kT + t) * 2], ai = tc[(k * kT + t) * 2 + 1];
        const float4 yr = *reinterpret_cast<const float4*>(&ys[wave][k][0][fr][a]);
        const float4 yi = *reinterpret_cast<const float4*>(&ys[wave][k][1][fr][a]);
        const float c0 = im ? ai : ar, c1 = im ? ar : -ai;       // re: ar yr - ai yi, im: ai yr + ar yi
        o.x += c0 * yr.x + c1 * yi.x;
        o.y += c0 * yr.y + c1 * yi.y;
        o.z += c0 * yr.z + c1 * yi.z;
        o.w += c0 * yr.w + c1 * yi.w;
      }
      *reinterpret_cast<float4*>(dst + e) = o;
    }
  } else {
    for (int e = lane; e < n; e += 64) {
      const int fr = e / rowlen, rem = e - fr * rowlen;
      const int t = rem / A2, c = rem - t * A2;
      const bool im = c >= A;
      const int a = im ? c - A : c;
      float o = 0.0f;
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        const float ar = tc[(k * kT + t) * 2], ai = tc[(k * kT + t) * 2 + 1];
        const float c0 = im ? ai : ar, c1 = im ? ar : -ai;
        o += c0 * ys[wave][k][0][fr][a] + c1 * ys[wave][k][1][fr][a];
      }
      dst[e] = o;
    }
  }
}

template <int ND>
void launch3_nd(const Chest3Args& a, bool vec, hipStream_t st) {
  const int Pmax = (a.F + 1) / 2;
  const int qtiles = (Pmax + 15) / 16, ftiles = (a.F + 15) / 16;
  k_chest3_pilot<ND><<<dim3(a.B * a.U, (qtiles + kChWaves - 1) / kChWaves), kChBlock, 0, st>>>(a);
  const dim3 grid(a.B * a.U, (ftiles + kChWaves - 1) / kChWaves);
  if (vec) k_chest3_expand<ND, true><<<grid, kChBlock, 0, st>>>(a);
  else k_chest3_expand<ND, false><<<grid, kChBlock, 0, st>>>(a);
}

ChestArgs chest_args(const nrx_chest_io& io) {
  ChestArgs a;
  a.B = io.batch;
  a.U = io.num_tx;
  a.F = io.num_subcarriers;
  a.A = io.num_rx_ant;
  a.nd = io.num_dmrs_symbols;
  for (int k = 0; k < 4; ++k) a.dm[k] = k < a.nd ? io.dmrs_symbols[k] : io.dmrs_symbols[0];
  a.grp_mask = 0;
  for (int u = 0; u < io.num_tx; ++u) a.grp_mask |= (unsigned)(io.cdm_group[u] & 1) << u;
  a.hh = io.h_hat;
  a.active = io.active;
  a.filt = io.filt;
  a.tcoef = io.tcoef;
  a.vconj = io.vconj;
  a.out = io.h_out;
  return a;
}

template <int ND>
void launch_nd(const ChestArgs& a, bool vec, hipStream_t st) {
  const int tiles = (a.F + 15) / 16;
  const dim3 grid(a.B * a.U, (tiles + kChWaves - 1) / kChWaves);
  if (vec) k_chest_lmmse<ND, true><<<grid, kChBlock, 0, st>>>(a);
  else k_chest_lmmse<ND, false><<<grid, kChBlock, 0, st>>>(a);
}

}  // namespace

size_t cov_workspace_bytes(const nrx_cov_io& io) {
  return (size_t)cov_groups(io) * (io.num_subcarriers + kT) * 2 * sizeof(double);
}

hipError_t launch_cov_accumulate(const nrx_cov_io& io, void* ws, hipStream_t st) {
  CovArgs a;
  a.F = io.num_subcarriers;
  a.A = io.num_rx_ant;
  a.groups = cov_groups(io);
  a.rows_f = (int64_t)io.batch * io.num_tx * kT * io.num_rx_ant;
  a.cols_t = (int64_t)io.batch * io.num_tx * io.num_subcarriers * io.num_rx_ant;
  a.h = io.h;
  a.part = (double*)ws;
  a.acc = io.acc;
  k_cov_partial<<<a.groups, kCovBlock, 0, st>>>(a);
  const int n = (a.F + kT) * 2;
  k_cov_reduce<<<(n + kCovBlock - 1) / kCovBlock, kCovBlock, 0, st>>>(a);
  return hipGetLastError();
}

size_t cov_space_workspace_bytes(const nrx_cov_space_io& io) {
  return (size_t)cov_space_groups(io) * io.num_rx_ant * io.num_rx_ant * 2 * sizeof(double);
}

hipError_t launch_cov_space(const nrx_cov_space_io& io, void* ws, hipStream_t st) {
  CovSpaceArgs a;
  a.A = io.num_rx_ant;
  a.groups = cov_space_groups(io);
  a.rows = (int64_t)io.batch * io.num_tx * io.num_subcarriers * kT;
  a.h = io.h;
  a.part = (double*)ws;
  a.acc = io.acc;
  k_cov_space_partial<<<a.groups, kCovBlock, 0, st>>>(a);
  const int n = a.A * a.A * 2;
  k_cov_space_reduce<<<(n + kCovBlock - 1) / kCovBlock, kCovBlock, 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_chest_lmmse(const nrx_chest_io& io, hipStream_t st) {
  const ChestArgs a = chest_args(io);
  // dwordx4 stores need A % 4 == 0 and a 16-byte aligned h_out (tiles start at multiples of 8A floats)
  const bool vec = io.num_rx_ant % 4 == 0 && ((uintptr_t)io.h_out & 15) == 0;
  switch (a.nd) {
    case 1: launch_nd<1>(a, vec, st); break;
    case 2: launch_nd<2>(a, vec, st); break;
    case 3: launch_nd<3>(a, vec, st); break;
    case 4: launch_nd<4>(a, vec, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

size_t chest3_workspace_bytes(const nrx_chest3_io& io) {
  const size_t Pmax = ((size_t)io.num_subcarriers + 1) / 2;
  return (size_t)io.batch * io.num_tx * Pmax * io.num_dmrs_symbols * 2 * io.num_rx_ant * sizeof(float);
}

hipError_t launch_chest_lmmse3(const nrx_chest3_io& io, void* ws, hipStream_t st) {
  Chest3Args a;
  a.B = io.batch;
  a.U = io.num_tx;
  a.F = io.num_subcarriers;
  a.A = io.num_rx_ant;
  a.nd = io.num_dmrs_symbols;
  for (int k = 0; k < 4; ++k) a.dm[k] = k < a.nd ? io.dmrs_symbols[k] : io.dmrs_symbols[0];
  a.grp_mask = 0;
  for (int u = 0; u < io.num_tx; ++u) a.grp_mask |= (unsigned)(io.cdm_group[u] & 1) << u;
  a.sigma2 = (float)(io.no / 2.0);
  a.hh = io.h_hat;
  a.active = io.active;
  a.qh = io.qh;
  a.gf = io.gf;
  a.nu = io.nu;
  a.tcoef = io.tcoef;
  a.vconj = io.vconj;
  a.lam = io.lam;
  a.vs = io.vs;
  a.mu = io.mu;
  a.cw = (float*)ws;
  a.out = io.h_out;
  const bool vec = io.num_rx_ant % 4 == 0 && ((uintptr_t)io.h_out & 15) == 0;
  switch (a.nd) {
    case 1: launch3_nd<1>(a, vec, st); break;
    case 2: launch3_nd<2>(a, vec, st); break;
    case 3: launch3_nd<3>(a, vec, st); break;
    case 4: launch3_nd<4>(a, vec, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_chest_lin(const nrx_chest_io& io, hipStream_t st) {
  const ChestArgs a = chest_args(io);
  const bool vec = io.num_rx_ant % 4 == 0 && (((uintptr_t)io.h_out | (uintptr_t)io.h_hat) & 15) == 0;
  const int64_t nvec = (int64_t)a.B * a.U * a.F * kT * (2 * a.A / (vec ? 4 : 1));
  const unsigned grid = (unsigned)((nvec + kChBlock - 1) / kChBlock);
  if (vec) k_chest_lin<true><<<grid, kChBlock, 0, st>>>(a, nvec);
  else k_chest_lin<false><<<grid, kChBlock, 0, st>>>(a, nvec);
  return hipGetLastError();
}

}  // namespace nrx
