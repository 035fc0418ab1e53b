// nrx_kbest.hip -- K-best MIMO detector on the GPU (nrx_kbest_detect, include/nrx.h): the detector
// of the reference's baseline_lmmse_kbest / baseline_perf_csi_kbest systems
// (utils/baseline_rx.py:242-254, KBestDetector with k = 64), defined here as a real-valued
// breadth-first tree search (include/nrx.h has the definition, tests/kbest_ref.py its numpy
// statement).
//
// Two kernels per call:
//
//   k_kbest_gram    one lane per RE, shaped like k_lmmse: the antennas stream through while the
//                   complex Gram matrix H^H H and H^H y accumulate in registers; U^2 + 2U floats
//                   per data RE go to the workspace.  The same lanes write the zeros of the
//                   DMRS symbols and of the inactive users, so the search only ever stores the
//                   rows of active users on data symbols.
//   k_kbest_search  one wave per data RE, lane = survivor (K <= 64 = the wave width).  The wave
//                   orders the users, expands the Gram matrix to its real 2n x 2n form in LDS,
//                   factorises it with lane j holding column j in registers (every pivot row
//                   is broadcast with v_readlane, so the factorisation touches no memory), and
//                   runs the 2n levels.  A lane holds a path as packed 3-bit level indices
//                   (16 x 3 = 48 bits) and its metric; the interference sum of a level is
//                   rebuilt from the packed path (R, y~ and the PAM tables are wave-uniform LDS
//                   reads), which costs the same O(n) per level as an incrementally updated
//                   residual vector but leaves three registers to move when survivors are
//                   compacted.  The K smallest of the <= 512 children of a level are selected by
//                   a bitwise radix select on the (non-negative) float bit patterns with
//                   __ballot + popcount; ties at the K-th place go to the lower (lane, child),
//                   so the selection is deterministic.  Survivors are compacted through mbcnt
//                   prefixes and a 64-entry LDS slot list, and each new lane re-derives its
//                   metric from its parent's state with the same child_metric() the selection
//                   used.  The final per-bit minima are taken by one lane per (user, bit) over
//                   the survivor list in LDS, and that lane stores its LLR.
//
// Every branch of the search is on wave-uniform values (n, L of the level, the survivor count).
// f32 throughout, no atomics, no allocation: outputs are bit-identical from call to call and do
// not depend on how slots are batched (every RE is handled on its own).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nrx.h"
#include "nrx_internal.h"

namespace nrx {

namespace {

constexpr int kGramBlock = 256;
constexpr int kWave = 64;
constexpr int kMaxStreams = 16;           // 2 * 8 users
constexpr int kRow = kMaxStreams + 1;     // a row of R plus its y~ entry
constexpr float kPivotMin = 1e-6f;        // pivot d_i <= kPivotMin * G_ii: the RE's LLRs are 0
constexpr int kSearchGridMax = 1 << 16;

struct KbestArgs {
  int64_t n;          // B * F * T
  int64_t nd;         // B * F * (data symbols)
  int F, FT, A, U, BS, dmrs_mask, num_mcs, K;
  int ndata;          // data symbols per slot
  int stride;         // workspace floats per RE: U^2 + 2U rounded up to 4
  int vst;            // llr rows may take vector stores (16-byte aligned base)
  int mcs_bits[8];
  int data_t[kT];     // the data symbols, ascending
  float inv_s, clip;
  const float* y;
  const float* h;
  const float* active;
  const uint8_t* mcs;
  float* llr;
  float* ws;
};

__host__ __device__ __forceinline__ int kbest_stride(int U) { return (U * U + 2 * U + 3) & ~3; }

__host__ __device__ __forceinline__ void zero_row(float* dst, int BS, bool vst) {
  if (vst && BS == 4) {
    *reinterpret_cast<float4*>(dst) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  } else if (vst && BS == 6) {
    *reinterpret_cast<float2*>(dst) = make_float2(0.0f, 0.0f);
    *reinterpret_cast<float2*>(dst + 2) = make_float2(0.0f, 0.0f);
    *reinterpret_cast<float2*>(dst + 4) = make_float2(0.0f, 0.0f);
  } else {
    for (int k = 0; k < BS; ++k) dst[k] = 0.0f;
  }
}

// RE i = (b * F + f) * T + t of the batch.  Data RE: the complex Gram matrix of all U columns
// (inactive ones included; the search leaves them out) and H^H y to the workspace -- entry
// [r][c], c < r: Re g_rc, entry [c][r]: Im g_rc with g_rc = h_r^H h_c, entry [r][r]: |h_r|^2,
// then (Re, Im) of h_r^H y -- and zeros to the LLR rows of the inactive users.  DMRS RE: zeros to
// every LLR row.  Host-callable too, so that the arithmetic can be stepped through without a
// device.
template <int U, bool VEC>
__host__ __device__ __forceinline__ void kbest_gram_re(const KbestArgs& p, int64_t i) {
  const int64_t b = i / p.FT;
  const int ft = (int)(i - b * p.FT);
  const int t = ft % kT;
  const int A = p.A;
  const bool data = !((p.dmrs_mask >> t) & 1);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!data || !(p.active[b * U + u] > 0.0f))
      zero_row(p.llr + (((size_t)b * U + u) * p.FT + ft) * p.BS, p.BS, p.vst != 0);
  }
  if (!data) return;

  float gr[U][U], gi[U][U], zr[U], zi[U];
#pragma unroll
  for (int r = 0; r < U; ++r) {
    zr[r] = zi[r] = 0.0f;
#pragma unroll
    for (int c = 0; c <= r; ++c) gr[r][c] = gi[r][c] = 0.0f;
  }
  const float* yrow = p.y + (size_t)i * 2 * A;
  const size_t hplane = (size_t)p.FT * 2 * A;                        // one (b, u) plane of h
  const float* hrow = p.h + (size_t)b * U * hplane + (size_t)ft * 2 * A;
  auto accumulate = [&](const float (&hr)[U], const float (&hi)[U], float yr, float yi) {
#pragma unroll
    for (int r = 0; r < U; ++r) {
      zr[r] += hr[r] * yr + hi[r] * yi;
      zi[r] += hr[r] * yi - hi[r] * yr;
#pragma unroll
      for (int c = 0; c < r; ++c) {
        gr[r][c] += hr[r] * hr[c] + hi[r] * hi[c];
        gi[r][c] += hr[r] * hi[c] - hi[r] * hr[c];
      }
      gr[r][r] += hr[r] * hr[r] + hi[r] * hi[r];
    }
  };
  if (VEC) {
    // two antennas per step (dwordx2): with four, U = 8 would hold 64 more floats in flight
    for (int a0 = 0; a0 < A; a0 += 2) {
      const float2 y2r = *reinterpret_cast<const float2*>(yrow + a0);
      const float2 y2i = *reinterpret_cast<const float2*>(yrow + A + a0);
      float2 h2r[U], h2i[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        h2r[u] = *reinterpret_cast<const float2*>(hrow + u * hplane + a0);
        h2i[u] = *reinterpret_cast<const float2*>(hrow + u * hplane + A + a0);
      }
      float hr[U], hi[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        hr[u] = h2r[u].x;
        hi[u] = h2i[u].x;
      }
      accumulate(hr, hi, y2r.x, y2i.x);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        hr[u] = h2r[u].y;
        hi[u] = h2i[u].y;
      }
      accumulate(hr, hi, y2r.y, y2i.y);
    }
  } else {
    for (int a = 0; a < A; ++a) {
      float hr[U], hi[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        hr[u] = hrow[u * hplane + a];
        hi[u] = hrow[u * hplane + A + a];
      }
      accumulate(hr, hi, yrow[a], yrow[A + a]);
    }
  }
  constexpr int S = (U * U + 2 * U + 3) & ~3;
  float w[S];
#pragma unroll
  for (int e = 0; e < S; ++e) w[e] = 0.0f;
#pragma unroll
  for (int r = 0; r < U; ++r) {
    w[r * U + r] = gr[r][r];
#pragma unroll
    for (int c = 0; c < r; ++c) {
      w[r * U + c] = gr[r][c];
      w[c * U + r] = gi[r][c];
    }
    w[U * U + 2 * r] = zr[r];
    w[U * U + 2 * r + 1] = zi[r];
  }
  float* dst = p.ws + (size_t)i * S;       // 16-byte aligned: the base is, and S % 4 == 0
#pragma unroll
  for (int e = 0; e < S; e += 4) *reinterpret_cast<float4*>(dst + e) = make_float4(w[e], w[e + 1], w[e + 2], w[e + 3]);
}

template <int U, bool VEC>
__global__ __launch_bounds__(kGramBlock) void k_kbest_gram(KbestArgs p) {
  const int64_t i = (int64_t)blockIdx.x * kGramBlock + threadIdx.x;
  if (i < p.n) kbest_gram_re<U, VEC>(p, i);
}

// ---- search ---------------------------------------------------------------------------------

// level l of the 2^nb-PAM of one axis, scaled to the unit-energy QAM; bit q of l is the axis'
// q-th bit (TS 38.211 5.1.3-5.1.5)
__device__ __forceinline__ float pam_amp(int nb, int l) {
  const float s0 = 1.0f - 2.0f * (float)(l & 1);
  const float s1 = 1.0f - 2.0f * (float)((l >> 1) & 1);
  const float s2 = 1.0f - 2.0f * (float)((l >> 2) & 1);
  const float v = nb == 1 ? s0 : (nb == 2 ? s0 * (2.0f - s1) : s0 * (4.0f - s1 * (2.0f - s2)));
  const float sc = nb == 1 ? 0.70710678118654752f : (nb == 2 ? 0.31622776601683794f : 0.15430334996209191f);
  return l < (1 << nb) ? v * sc : 0.0f;
}

// metric of the child with amplitude a of a path with metric lam and residual r at a level whose
// diagonal entry is rii.  One definition with explicit roundings: the lane that selects a child and
// the lane that adopts it compute the same bits.
__device__ __forceinline__ float child_metric(float lam, float r, float rii, float a, float inv_s) {
  const float e = __fmaf_rn(-rii, a, r);
  return __fmaf_rn(__fmul_rn(e, e), inv_s, lam);
}

__device__ __forceinline__ float lane_bcast(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// lanes below this one whose bit is set in the ballot
__device__ __forceinline__ int mask_rank(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// exclusive prefix over the wave of a count 0..15
__device__ __forceinline__ int wave_prefix4(int v) {
  int pre = 0;
#pragma unroll
  for (int bit = 0; bit < 4; ++bit) pre += mask_rank(__ballot((v >> bit) & 1)) << bit;
  return pre;
}

__global__ __launch_bounds__(kWave) void k_kbest_search(KbestArgs p) {
  __shared__ float sW[84];                    // the RE's workspace record (<= 80 floats)
  __shared__ float sR[kMaxStreams * kRow];    // real Gram matrix, then R | y~
  __shared__ float sAmp[kMaxStreams * 8];     // PAM levels of every stream
  __shared__ int sPerm[8], sBits[8];          // p-th user of the order: port, bits
  __shared__ int sSlot[kWave];                // survivor list: parent lane << 3 | child
  __shared__ float sLam[kWave];
  __shared__ unsigned sLo[kWave], sHi[kWave];
  __shared__ int sT[16];

  const int lane = threadIdx.x;
  const int U = p.U;
  const float inf = __int_as_float(0x7f800000);
#pragma unroll
  for (int k = 0; k < kT; ++k)
    if (lane == k) sT[k] = p.data_t[k];

  for (int64_t j = blockIdx.x; j < p.nd; j += gridDim.x) {
    const int64_t b = j / ((int64_t)p.F * p.ndata);
    const int rem = (int)(j - b * ((int64_t)p.F * p.ndata));
    const int f = rem / p.ndata;
    __syncthreads();                          // the previous RE's LDS reads are done; sT is written
    const int ft = f * kT + sT[rem - f * p.ndata];
    const int64_t i = b * p.FT + ft;

    for (int e = lane; e < p.stride; e += kWave) sW[e] = p.ws[(size_t)i * p.stride + e];
    bool act = false;
    int bits = 2;
    if (lane < U) {
      act = p.active[b * U + lane] > 0.0f;
      int mi = p.mcs ? (int)p.mcs[b * U + lane] : 0;
      mi = mi < p.num_mcs ? mi : p.num_mcs - 1;
      bits = p.mcs_bits[mi];
    }
    if (lane < 8) {
      sPerm[lane] = 0;
      sBits[lane] = 2;
    }
    const unsigned actmask = (unsigned)__ballot(act);
    const int n = __popc(actmask);
    const int n2 = 2 * n;
    __syncthreads();
    // order: |h_u|^2 ascending, ties to the lower port
    if (act) {
      const float mine = sW[lane * U + lane];
      int rank = 0;
      for (int v = 0; v < U; ++v) {
        const float other = sW[v * U + v];
        rank += ((actmask >> v) & 1) && (other < mine || (other == mine && v < lane)) ? 1 : 0;
      }
      sPerm[rank & 7] = lane;
      sBits[rank & 7] = bits;
    }
    __syncthreads();
    // real Gram matrix in stream order [Re u(1), Im u(1), Re u(2), ...], column 16 = H^T y_r
    for (int e = lane; e < kMaxStreams * kRow; e += kWave) {
      const int r = e / kRow, c = e - r * kRow;
      float val = 0.0f;
      if (r < n2) {
        const int u = sPerm[r >> 1], ar = r & 1;
        if (c == kMaxStreams) {
          val = sW[U * U + 2 * u + ar];
        } else if (c < n2) {
          const int v = sPerm[c >> 1], ac = c & 1;
          if (u == v) {
            val = ar == ac ? sW[u * U + u] : 0.0f;
          } else {
            const int hi = u > v ? u : v, lo = u > v ? v : u;
            const float re = sW[hi * U + lo];
            const float im = u > v ? sW[lo * U + hi] : -sW[lo * U + hi];      // Im(h_u^H h_v)
            val = ar == ac ? re : (ar == 0 ? -im : im);
          }
        }
      }
      sR[e] = val;
    }
    for (int e = lane; e < kMaxStreams * 8; e += kWave) {
      const int st = e >> 3;
      sAmp[e] = st < n2 ? pam_amp(sBits[st >> 1] >> 1, e & 7) : 0.0f;
    }
    __syncthreads();
    // G = R^T R, y~ = R^-T z: lane c holds column c (lane 16 the right-hand side); row k of R is
    // final once step k is done, so step i reads R_ki from lane i
    const int col_id = lane < kMaxStreams ? lane : kMaxStreams;
    float col[kMaxStreams];
#pragma unroll
    for (int k = 0; k < kMaxStreams; ++k) col[k] = sR[k * kRow + col_id];
    bool degen = n == 0;
#pragma unroll
    for (int s = 0; s < kMaxStreams; ++s) {
      if (s < n2) {
        const float gii = lane_bcast(col[s], s);
        float num = col[s];
#pragma unroll
        for (int k = 0; k < s; ++k) num = __fmaf_rn(-lane_bcast(col[k], s), col[k], num);
        const float d = lane_bcast(num, s);
        const bool bad = !(d > kPivotMin * gii);
        degen = degen || bad;
        const float rii = __fsqrt_rn(bad ? 1.0f : d);
        col[s] = lane == s ? rii : __fdiv_rn(num, rii);
      }
    }
    if (lane <= kMaxStreams) {
#pragma unroll
      for (int k = 0; k < kMaxStreams; ++k) sR[k * kRow + lane] = col[k];
    }
    __syncthreads();

    float lam = lane == 0 ? 0.0f : inf;
    unsigned long long path = 0;
    int C = 1;
    if (!degen) {
      for (int s = n2 - 1; s >= 0; --s) {
        const int nb = sBits[s >> 1] >> 1;
        const int L = 1 << nb;
        float r = sR[s * kRow + kMaxStreams];
        for (int c = s + 1; c < n2; ++c)
          r = __fmaf_rn(-sR[s * kRow + c], sAmp[c * 8 + ((unsigned)(path >> (3 * c)) & 7u)], r);
        const float rii = sR[s * kRow + s];
        int slot, Cn;
        if (C * L > p.K) {
          // the K smallest of the C * L children
          unsigned key[8];
#pragma unroll
          for (int l = 0; l < 8; ++l) {
            const float m = child_metric(lam, r, rii, sAmp[s * 8 + l], p.inv_s);
            key[l] = (lane < C && l < L) ? (unsigned)__float_as_int(m) : 0xffffffffu;
          }
          unsigned alive = 0xffu;               // children whose key matches the prefix so far
          int need = p.K;
          unsigned thr = 0;
          for (int bit = 31; bit >= 0; --bit) {
            int cnt0 = 0;
#pragma unroll
            for (int l = 0; l < 8; ++l)
              if (l < L) cnt0 += __popcll(__ballot(((alive >> l) & 1u) && !((key[l] >> bit) & 1u)));
            const bool one = need > cnt0;
            if (one) {
              need -= cnt0;
              thr |= 1u << bit;
            }
#pragma unroll
            for (int l = 0; l < 8; ++l)
              if (((key[l] >> bit) & 1u) != (one ? 1u : 0u)) alive &= ~(1u << l);
          }
          // keys below thr are in; of the keys equal to thr the first `need` in (lane, child) order
          int ne = 0;
#pragma unroll
          for (int l = 0; l < 8; ++l) ne += key[l] == thr ? 1 : 0;
          int eq_rank = wave_prefix4(ne);
          unsigned take = 0;
          int ct = 0;
#pragma unroll
          for (int l = 0; l < 8; ++l) {
            bool in = key[l] < thr;
            if (key[l] == thr) {
              in = eq_rank < need;
              ++eq_rank;
            }
            take |= in ? 1u << l : 0u;
            ct += in ? 1 : 0;
          }
          int dst = wave_prefix4(ct);
#pragma unroll
          for (int l = 0; l < 8; ++l) {
            if ((take >> l) & 1u) {
              sSlot[dst & (kWave - 1)] = (lane << 3) | l;
              ++dst;
            }
          }
          Cn = p.K;
          __syncthreads();
          slot = sSlot[lane];
          __syncthreads();
        } else {
          Cn = C * L;
          slot = ((lane >> nb) << 3) | (lane & (L - 1));
        }
        const int par = (slot >> 3) & (kWave - 1), ch = slot & 7;
        const float lp = __shfl(lam, par);
        const float rp = __shfl(r, par);
        const unsigned plo = __shfl((unsigned)path, par);
        const unsigned phi = __shfl((unsigned)(path >> 32), par);
        const float m = child_metric(lp, rp, rii, sAmp[s * 8 + ch], p.inv_s);
        lam = lane < Cn ? m : inf;
        path = (((unsigned long long)phi << 32) | plo) | ((unsigned long long)ch << (3 * s));
        C = Cn;
      }
    }
    sLam[lane] = lam;
    sLo[lane] = (unsigned)path;
    sHi[lane] = (unsigned)(path >> 32);
    __syncthreads();
    // lane (pos, kb): bit kb of the pos-th user of the order
    const int pos = lane >> 3, kb = lane & 7;
    if (pos < n) {
      const int u = sPerm[pos], m = sBits[pos];
      float v = 0.0f;
      if (!degen && kb < m) {
        const int sh = 3 * (2 * pos + (kb & 1)) + (kb >> 1);
        float m0 = inf, m1 = inf;
        for (int q = 0; q < C; ++q) {
          const unsigned long long pq = ((unsigned long long)sHi[q] << 32) | sLo[q];
          const float lq = sLam[q];
          if ((pq >> sh) & 1ull) m1 = fminf(m1, lq);
          else m0 = fminf(m0, lq);
        }
        v = fminf(fmaxf(m0 - m1, -p.clip), p.clip);
      }
      float* dst = p.llr + (((size_t)b * U + u) * p.FT + ft) * p.BS;
      if (kb < p.BS) dst[kb] = v;
      if (kb == 7)
        for (int k = 8; k < p.BS; ++k) dst[k] = 0.0f;
    }
  }
}

template <int U>
void launch_gram(const KbestArgs& a, bool vec, hipStream_t st) {
  const unsigned grid = (unsigned)((a.n + kGramBlock - 1) / kGramBlock);
  if (vec) k_kbest_gram<U, true><<<grid, kGramBlock, 0, st>>>(a);
  else k_kbest_gram<U, false><<<grid, kGramBlock, 0, st>>>(a);
}

}  // namespace

size_t kbest_workspace_bytes(const nrx_kbest_io& io) {
  return (size_t)io.batch * io.num_subcarriers * io.num_symbols * kbest_stride(io.num_tx) * sizeof(float);
}

hipError_t launch_kbest(const nrx_kbest_io& io, void* ws, hipStream_t st) {
  KbestArgs a;
  a.F = io.num_subcarriers;
  a.FT = io.num_subcarriers * io.num_symbols;
  a.n = (int64_t)io.batch * a.FT;
  a.A = io.num_rx_ant;
  a.U = io.num_tx;
  a.BS = io.bits_stride;
  a.dmrs_mask = io.dmrs_symbol_mask;
  a.num_mcs = io.num_mcs;
  a.K = io.k;
  a.ndata = 0;
  for (int t = 0; t < kT; ++t) {
    a.data_t[t] = 0;
    if (!((io.dmrs_symbol_mask >> t) & 1)) a.data_t[a.ndata++] = t;
  }
  a.nd = (int64_t)io.batch * io.num_subcarriers * a.ndata;
  a.stride = kbest_stride(io.num_tx);
  for (int m = 0; m < 8; ++m) a.mcs_bits[m] = m < io.num_mcs ? io.mcs_bits[m] : io.mcs_bits[0];
  a.inv_s = (float)(1.0 / (io.no + io.err_var));
  a.clip = (float)io.llr_clip;
  a.y = io.y;
  a.h = io.h;
  a.active = io.active;
  a.mcs = io.mcs;
  a.llr = io.llr;
  a.ws = (float*)ws;
  // dwordx2 loads need an even A and 8-byte aligned bases (rows are 8A bytes); else scalar loads
  const bool vec = io.num_rx_ant % 2 == 0 && (((uintptr_t)io.y | (uintptr_t)io.h) & 7) == 0;
  a.vst = ((uintptr_t)io.llr & 15) == 0;
  switch (io.num_tx) {
    case 1: launch_gram<1>(a, vec, st); break;
    case 2: launch_gram<2>(a, vec, st); break;
    case 3: launch_gram<3>(a, vec, st); break;
    case 4: launch_gram<4>(a, vec, st); break;
    case 5: launch_gram<5>(a, vec, st); break;
    case 6: launch_gram<6>(a, vec, st); break;
    case 7: launch_gram<7>(a, vec, st); break;
    case 8: launch_gram<8>(a, vec, st); break;
    default: return hipErrorInvalidValue;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.nd == 0) return e;
  const unsigned grid = (unsigned)(a.nd < kSearchGridMax ? a.nd : kSearchGridMax);
  k_kbest_search<<<grid, kWave, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace nrx
