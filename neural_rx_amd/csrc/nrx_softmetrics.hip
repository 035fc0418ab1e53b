// nrx_softmetrics.hip -- soft-output metrics of an evaluation loop (include/nrx.h): the bitwise
// mutual-information loss sums of a batch of LLRs (nrx_llr_stats) and the squared-error sums of a
// channel estimate (nrx_chest_nmse).
//
// Both run as two launches.  The first has one workgroup per item = (slot b, user u, strip of at
// most kSoftFS subcarriers): a strip is one contiguous run of kSoftFS * 14 resource elements, one
// per lane for the LLRs.  The lanes' float64 terms are reduced across the wave with the __shfl_xor
// ladder, then across the four waves through LDS in a fixed order, and one partial record per item
// goes to the workspace.  An item of an inactive (slot, user) exits after its load of `active` and
// writes nothing.  The second launch has one workgroup per user; thread e owns element e of the
// record and adds the active items' partials in ascending (b, strip) order into the accumulator row
// of the slot's MCS.  The partition depends on the shape only and nothing is added atomically, so
// the same inputs give the same bits on every call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nrx.h"
#include "nrx_internal.h"

namespace nrx {

namespace {

constexpr int kSoftBlock = 256;
constexpr int kSoftWaves = kSoftBlock / 64;
constexpr int kMaxBits = 8;          // k axis of the accumulators
constexpr int kMaxScales = 16;
constexpr int kRedTileElems = 7168;  // 8-byte elements of LLR partial records the ordered pass stages in LDS (56 KB)
constexpr int kRedRecords = 512;     // and at most this many records
constexpr int kRedBlock = 1024;      // threads of the LLR ordered pass: sixteen waves load a tile together
constexpr int kRedWaves = kRedBlock / 64;
constexpr int kRedBatch = 16;        // staged records a thread reads from LDS ahead of adding them
constexpr int kRedSlots = 256;      // slots whose (active, MCS) the ordered pass stages at a time
static_assert(kSoftFS * kT <= kSoftBlock, "one resource element per lane");

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// N sums at once: the ladders are independent, so their cross-lane moves overlap
template <class T, int N>
__device__ __forceinline__ void wave_sum(T (&v)[N]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], o);
  }
}

// ------------------------------------------------------------------ LLR statistics
struct LlrArgs {
  int B, U, F, H, BS, M, S, NS;     // NS strips per (b, u)
  int mcs_bits[8];
  int dmrs_mask;
  double scales[kMaxScales];
  const float* llr;
  const uint8_t* bits;
  const uint8_t* mcs;
  const float* active;
  double* ws;                        // [B * U * NS] records: [8][S] f64 loss (bits), [8] i64 cnt, [8] i64 nonfinite
  double* loss;
  long long* cnt;
  long long* nonfinite;
};

// one row of BSC LLRs / sent bits as vector loads (rows are BSC * 4 / BSC bytes apart and the
// launcher checks the base alignment); BSC = 0: any stride, the first nb entries one by one
template <int BSC>
__device__ __forceinline__ void load_row(const float* l, const uint8_t* c, int stride, int nb, float (&lv)[kMaxBits],
                                         unsigned (&cv)[kMaxBits]) {
  if constexpr (BSC == 4) {
    const float4 v = *reinterpret_cast<const float4*>(l);
    const unsigned w = *reinterpret_cast<const unsigned*>(c);
    lv[0] = v.x, lv[1] = v.y, lv[2] = v.z, lv[3] = v.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) cv[k] = (w >> (8 * k)) & 0xffu;
  } else if constexpr (BSC == 8) {
    const float4 v0 = reinterpret_cast<const float4*>(l)[0], v1 = reinterpret_cast<const float4*>(l)[1];
    const uint2 w = *reinterpret_cast<const uint2*>(c);
    lv[0] = v0.x, lv[1] = v0.y, lv[2] = v0.z, lv[3] = v0.w;
    lv[4] = v1.x, lv[5] = v1.y, lv[6] = v1.z, lv[7] = v1.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cv[k] = (w.x >> (8 * k)) & 0xffu;
      cv[4 + k] = (w.y >> (8 * k)) & 0xffu;
    }
  } else if constexpr (BSC == 2 || BSC == 6) {
#pragma unroll
    for (int q = 0; q < BSC / 2; ++q) {
      const float2 v = reinterpret_cast<const float2*>(l)[q];
      const unsigned w = reinterpret_cast<const unsigned short*>(c)[q];
      lv[2 * q] = v.x, lv[2 * q + 1] = v.y;
      cv[2 * q] = w & 0xffu, cv[2 * q + 1] = w >> 8;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kMaxBits; ++k) {
      lv[k] = k < nb ? l[k] : 0.0f;
      cv[k] = k < nb ? c[k] : 0u;
    }
  }
}

template <int BSC>
__global__ __launch_bounds__(kSoftBlock) void k_llr_partial(LlrArgs p) {
  constexpr int KN = BSC ? BSC : kMaxBits;
  __shared__ double red[kSoftWaves][kMaxBits * kMaxScales];
  __shared__ unsigned redi[kSoftWaves][2 * kMaxBits];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t item = blockIdx.x;
  const int strip = (int)(item % p.NS);
  const int64_t bu = item / p.NS;
  if (!(p.active[bu] > 0.0f)) return;                  // uniform over the workgroup
  int m = p.mcs ? p.mcs[bu] : 0;
  m = m < p.M ? m : p.M - 1;
  const int nb = p.mcs_bits[m] < KN ? p.mcs_bits[m] : KN;
  const int head = p.H > 1 ? m : 0;
  const int stride = BSC ? BSC : p.BS;
  const int f0 = strip * kSoftFS;
  const int nre = (p.F - f0 < kSoftFS ? p.F - f0 : kSoftFS) * kT;
  const int i = tid < nre ? tid : nre - 1;             // lanes past the strip load its last RE, masked below
  const bool data = tid < nre && !((p.dmrs_mask >> (i % kT)) & 1);
  const int64_t re = (bu * p.F + f0) * kT + i;
  const float* l = p.llr + ((int64_t)head * p.B * p.U * p.F * kT + re) * stride;
  const uint8_t* c = p.bits + re * stride;
  float lv[kMaxBits];
  unsigned cv[kMaxBits];
  load_row<BSC>(l, c, stride, nb, lv, cv);

  bool fin[KN];
  double zl[KN];                                       // (2c - 1) L
  unsigned ni[2 * KN];                                 // finite, non-finite
#pragma unroll
  for (int k = 0; k < KN; ++k) {
    const bool in = data && k < nb;
    const bool f = isfinite(lv[k]);
    fin[k] = in && f;
    zl[k] = fin[k] ? (cv[k] ? (double)lv[k] : -(double)lv[k]) : 0.0;
    ni[k] = fin[k] ? 1u : 0u;
    ni[KN + k] = in && !f ? 1u : 0u;
  }
  wave_sum(ni);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < KN; ++k) {
      redi[wave][k] = ni[k];
      redi[wave][kMaxBits + k] = ni[KN + k];
    }
  }
  const int S = p.S;
  for (int s = 0; s < S; ++s) {
    const double sc = p.scales[s];
    double v[KN];
#pragma unroll
    for (int k = 0; k < KN; ++k) {
      v[k] = 0.0;
      if (k < nb && fin[k]) {
        const double z = zl[k] * sc;
        // the unbounded linear term in f64; the bounded one, in (0, ln 2], in f32
        v[k] = fmax(-z, 0.0) + (double)log1pf(expf((float)(-fabs(z))));
      }
    }
    wave_sum(v);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < KN; ++k) red[wave][k * S + s] = v[k];
    }
  }
  __syncthreads();
  double* rec = p.ws + item * (int64_t)(kMaxBits * S + 2 * kMaxBits);
  if (tid < kMaxBits * S) {
    const int k = tid / S;
    double t = 0.0;
    if (k < nb) t = (((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]) * 1.4426950408889634;   // 1 / ln 2
    rec[tid] = t;
  } else if (tid < kMaxBits * S + 2 * kMaxBits) {
    const int e = tid - kMaxBits * S;
    long long t = 0;
    if ((e & (kMaxBits - 1)) < nb) t = (long long)redi[0][e] + redi[1][e] + redi[2][e] + redi[3][e];
    reinterpret_cast<long long*>(rec)[tid] = t;
  }
}

// workgroup u.  Per chunk of kRedSlots slots the lanes first note the MCS row of every (b, u) (-1:
// inactive, its records were never written).  The workgroup then stages as many records as fit in
// LDS at a time -- wave w of the sixteen takes records w, w + 16, ..., a lane the elements lane,
// lane + 64, ..., so the loads of a tile are independent and in flight together -- and thread
// e < 8 S + 16 adds element e of the staged records in ascending (b, strip) order, one select per
// MCS row and record and no branch (MM >= num_mcs rows, a template argument).  The integer elements
// take the same float64 adds: an item counts at most 224 and a call's sum stays far below 2^53, so
// they are exact, and are converted back when they are added to the int64 accumulators.
template <int MM>
__global__ __launch_bounds__(kRedBlock) void k_llr_reduce(LlrArgs p) {
  __shared__ long long tile[kRedTileElems];
  __shared__ int s_m[kRedSlots];                       // MCS of (b, u), -1: inactive
  __shared__ int s_row[kRedRecords];                   // MCS row of a staged record, -1: inactive
  __shared__ int s_item[kRedRecords];                  // its item index
  constexpr int kLoadBatch = 4;
  constexpr int kRecPasses = (kMaxBits * kMaxScales + 2 * kMaxBits + 63) / 64;   // 64-lane passes over a record
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
  const int nd = kMaxBits * p.S, nrec = nd + 2 * kMaxBits;
  int R = kRedTileElems / nrec;                        // records per tile
  R = R < kRedRecords ? R : kRedRecords;
  const bool isd = tid < nd;
  double ds[MM];
#pragma unroll
  for (int r = 0; r < MM; ++r) ds[r] = 0.0;
  const long long* wsi = reinterpret_cast<const long long*>(p.ws);
  for (int b0 = 0; b0 < p.B; b0 += kRedSlots) {
    const int nbk = p.B - b0 < kRedSlots ? p.B - b0 : kRedSlots;
    __syncthreads();                                   // the previous chunk has been read
    if (tid < nbk) {
      const int64_t bu = (int64_t)(b0 + tid) * p.U + u;
      int m = -1;
      if (p.active[bu] > 0.0f) {
        m = p.mcs ? p.mcs[bu] : 0;
        m = m < p.M ? m : p.M - 1;
      }
      s_m[tid] = m;
    }
    __syncthreads();
    const int n = nbk * p.NS;
    for (int j0 = 0; j0 < n; j0 += R) {
      const int nj = n - j0 < R ? n - j0 : R;
      for (int q = tid; q < nj; q += kRedBlock) {
        const int j = j0 + q, jb = j / p.NS;
        s_row[q] = s_m[jb];
        s_item[q] = ((b0 + jb) * p.U + u) * p.NS + (j - jb * p.NS);   // < 2^31 (B, U, F limits of the entry point)
      }
      __syncthreads();
      // kLoadBatch records per wave and step, every load issued before the first LDS store
      for (int q0 = wave; q0 < nj; q0 += kRedWaves * kLoadBatch) {
        long long v[kLoadBatch][kRecPasses];
#pragma unroll
        for (int i = 0; i < kLoadBatch; ++i) {
          const int q = q0 + kRedWaves * i;
          const int qc = q < nj ? q : nj - 1;
          const bool on = q < nj && s_row[qc] >= 0;
          const long long* rec = wsi + (int64_t)s_item[qc] * nrec;
#pragma unroll
          for (int c = 0; c < kRecPasses; ++c) v[i][c] = on && lane + 64 * c < nrec ? rec[lane + 64 * c] : 0;
        }
#pragma unroll
        for (int i = 0; i < kLoadBatch; ++i) {
          const int q = q0 + kRedWaves * i;
#pragma unroll
          for (int c = 0; c < kRecPasses; ++c)
            if (q < nj && lane + 64 * c < nrec) tile[q * nrec + lane + 64 * c] = v[i][c];
        }
      }
      __syncthreads();
      if (tid < nrec) {
        for (int q0 = 0; q0 < nj; q0 += kRedBatch) {   // the LDS reads of a batch ahead of its dependent adds
          int mm[kRedBatch];
          long long raw[kRedBatch];
#pragma unroll
          for (int i = 0; i < kRedBatch; ++i) {
            const int q = q0 + i < nj ? q0 + i : nj - 1;
            mm[i] = q0 + i < nj ? s_row[q] : -1;
            raw[i] = tile[q * nrec + tid];
          }
#pragma unroll
          for (int i = 0; i < kRedBatch; ++i) {
            const double dv = isd ? __longlong_as_double(raw[i]) : (double)raw[i];
#pragma unroll
            for (int r = 0; r < MM; ++r) ds[r] += mm[i] == r ? dv : 0.0;
          }
        }
      }
      __syncthreads();                                 // the tile has been read
    }
  }
  if (tid >= nrec) return;
#pragma unroll
  for (int r = 0; r < MM; ++r) {
    if (r >= p.M) break;
    const int64_t row = (int64_t)u * p.M + r;
    if (isd) {
      p.loss[row * nd + tid] += ds[r];
    } else {
      const int e = tid - nd;                          // [0, 8): cnt, [8, 16): nonfinite
      long long* dst = e < kMaxBits ? p.cnt : p.nonfinite;
      dst[row * kMaxBits + (e & (kMaxBits - 1))] += (long long)ds[r];
    }
  }
}

// ------------------------------------------------------------------ channel NMSE
struct NmseArgs {
  int B, U, F, A, NS;
  int mask;                          // bit t: symbol t is selected
  const float* he;
  const float* h;
  const float* active;
  double* ws;                        // [B * U * NS][2]: err, ref
  double* err;
  double* ref;
  long long* items;
};

template <bool VEC>
__global__ __launch_bounds__(kSoftBlock) void k_nmse_partial(NmseArgs p) {
  __shared__ double red[kSoftWaves][2];
  const int tid = threadIdx.x;
  const int64_t item = blockIdx.x;
  const int strip = (int)(item % p.NS);
  const int64_t bu = item / p.NS;
  if (!(p.active[bu] > 0.0f)) return;                  // uniform over the workgroup
  const int A2 = 2 * p.A;
  const int f0 = strip * kSoftFS;
  const int n = (p.F - f0 < kSoftFS ? p.F - f0 : kSoftFS) * kT * A2;   // contiguous floats of the strip
  const int64_t base = (bu * p.F + f0) * (int64_t)kT * A2;
  const float* he = p.he + base;
  const float* h = p.h + base;
  double e = 0.0, r = 0.0;
  if (VEC) {                                           // A2 is even: a float2 never straddles two symbols
    for (int i = 2 * tid; i < n; i += 2 * kSoftBlock) {
      const float2 a = *reinterpret_cast<const float2*>(he + i), b = *reinterpret_cast<const float2*>(h + i);
      if (!((p.mask >> ((i / A2) % kT)) & 1)) continue;
      const double d0 = (double)a.x - (double)b.x, d1 = (double)a.y - (double)b.y;
      e += d0 * d0 + d1 * d1;
      r += (double)b.x * (double)b.x + (double)b.y * (double)b.y;
    }
  } else {
    for (int i = tid; i < n; i += kSoftBlock) {
      const float a = he[i], b = h[i];
      if (!((p.mask >> ((i / A2) % kT)) & 1)) continue;
      const double d = (double)a - (double)b;
      e += d * d;
      r += (double)b * (double)b;
    }
  }
  e = wave_sum(e);
  r = wave_sum(r);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = e;
    red[tid >> 6][1] = r;
  }
  __syncthreads();
  if (tid < 2) p.ws[item * 2 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// workgroup u; lane q stages record j0 + q of a tile of kSoftBlock records in LDS (0 for an inactive
// item, whose record was never written), then threads 0 / 1 add err / ref of the staged records in
// ascending (b, strip) order and thread 2 counts the items
__global__ __launch_bounds__(kSoftBlock) void k_nmse_reduce(NmseArgs p) {
  __shared__ int s_a[kRedSlots];
  __shared__ double tile[kSoftBlock][2];
  const int tid = threadIdx.x, u = blockIdx.x;
  double acc = 0.0;
  long long cnt = 0;
  for (int b0 = 0; b0 < p.B; b0 += kRedSlots) {
    const int nbk = p.B - b0 < kRedSlots ? p.B - b0 : kRedSlots;
    __syncthreads();
    if (tid < nbk) s_a[tid] = p.active[(int64_t)(b0 + tid) * p.U + u] > 0.0f ? 1 : 0;
    __syncthreads();
    if (tid == 2)
      for (int j = 0; j < nbk; ++j) cnt += s_a[j];
    const int n = nbk * p.NS;
    for (int j0 = 0; j0 < n; j0 += kSoftBlock) {
      const int nj = n - j0 < kSoftBlock ? n - j0 : kSoftBlock;
      if (tid < nj) {
        const int j = j0 + tid, jb = j / p.NS;
        const int64_t it = ((int64_t)(b0 + jb) * p.U + u) * p.NS + (j - jb * p.NS);
        const bool on = s_a[jb] != 0;
        tile[tid][0] = on ? p.ws[it * 2] : 0.0;
        tile[tid][1] = on ? p.ws[it * 2 + 1] : 0.0;
      }
      __syncthreads();
      if (tid < 2) {
        for (int q0 = 0; q0 < nj; q0 += kRedBatch) {   // the LDS reads of a batch ahead of its dependent adds
          double v[kRedBatch];
#pragma unroll
          for (int i = 0; i < kRedBatch; ++i) v[i] = q0 + i < nj ? tile[q0 + i][tid] : 0.0;
#pragma unroll
          for (int i = 0; i < kRedBatch; ++i) acc += v[i];
        }
      }
      __syncthreads();                                 // the tile has been read
    }
  }
  if (tid == 0) p.err[u] += acc;
  if (tid == 1) p.ref[u] += acc;
  if (tid == 2) p.items[u] += cnt;
}

int strips(int F) { return (F + kSoftFS - 1) / kSoftFS; }

}  // namespace

size_t llr_stats_workspace_bytes(const nrx_llr_stats_io& io) {
  return (size_t)io.batch * io.num_tx * strips(io.num_subcarriers) * (kMaxBits * io.num_scales + 2 * kMaxBits) * 8;
}

hipError_t launch_llr_stats(const nrx_llr_stats_io& io, void* ws, hipStream_t st) {
  LlrArgs p;
  p.B = io.batch, p.U = io.num_tx, p.F = io.num_subcarriers, p.H = io.num_heads, p.BS = io.bits_stride;
  p.M = io.num_mcs, p.S = io.num_scales, p.NS = strips(io.num_subcarriers);
  for (int m = 0; m < 8; ++m) p.mcs_bits[m] = m < io.num_mcs ? io.mcs_bits[m] : 0;
  p.dmrs_mask = io.dmrs_symbol_mask;
  for (int s = 0; s < kMaxScales; ++s) p.scales[s] = s < io.num_scales ? io.scales[s] : 0.0;
  p.llr = io.llr, p.bits = io.bits, p.mcs = io.mcs, p.active = io.active;
  p.ws = (double*)ws, p.loss = io.loss, p.cnt = (long long*)io.cnt, p.nonfinite = (long long*)io.nonfinite;
  const unsigned items = (unsigned)((int64_t)p.B * p.U * p.NS);
  // the vector rows need the row alignment at the base: 16 / 8 bytes of LLRs, 4 / 2 / 8 of bits
  const uintptr_t la = (uintptr_t)io.llr, ba = (uintptr_t)io.bits;
  int bsc = 0;
  if (io.bits_stride == 4 && !(la & 15) && !(ba & 3)) bsc = 4;
  if (io.bits_stride == 8 && !(la & 15) && !(ba & 7)) bsc = 8;
  if ((io.bits_stride == 2 || io.bits_stride == 6) && !(la & 7) && !(ba & 1)) bsc = io.bits_stride;
  switch (bsc) {
    case 2: k_llr_partial<2><<<items, kSoftBlock, 0, st>>>(p); break;
    case 4: k_llr_partial<4><<<items, kSoftBlock, 0, st>>>(p); break;
    case 6: k_llr_partial<6><<<items, kSoftBlock, 0, st>>>(p); break;
    case 8: k_llr_partial<8><<<items, kSoftBlock, 0, st>>>(p); break;
    default: k_llr_partial<0><<<items, kSoftBlock, 0, st>>>(p);
  }
  switch (p.M) {
    case 1: k_llr_reduce<1><<<p.U, kRedBlock, 0, st>>>(p); break;
    case 2: k_llr_reduce<2><<<p.U, kRedBlock, 0, st>>>(p); break;
    case 3: k_llr_reduce<3><<<p.U, kRedBlock, 0, st>>>(p); break;
    case 4: k_llr_reduce<4><<<p.U, kRedBlock, 0, st>>>(p); break;
    default: k_llr_reduce<8><<<p.U, kRedBlock, 0, st>>>(p);
  }
  return hipGetLastError();
}

size_t nmse_workspace_bytes(const nrx_nmse_io& io) {
  return (size_t)io.batch * io.num_tx * strips(io.num_subcarriers) * 2 * 8;
}

hipError_t launch_chest_nmse(const nrx_nmse_io& io, void* ws, hipStream_t st) {
  NmseArgs p;
  p.B = io.batch, p.U = io.num_tx, p.F = io.num_subcarriers, p.A = io.num_rx_ant, p.NS = strips(io.num_subcarriers);
  p.mask = io.symbol_mask ? io.symbol_mask : (1 << kT) - 1;
  p.he = io.h_est, p.h = io.h_true, p.active = io.active;
  p.ws = (double*)ws, p.err = io.err, p.ref = io.ref, p.items = (long long*)io.items;
  const unsigned items = (unsigned)((int64_t)p.B * p.U * p.NS);
  if (!(((uintptr_t)io.h_est | (uintptr_t)io.h_true) & 7))
    k_nmse_partial<true><<<items, kSoftBlock, 0, st>>>(p);
  else
    k_nmse_partial<false><<<items, kSoftBlock, 0, st>>>(p);
  k_nmse_reduce<<<p.U, kSoftBlock, 0, st>>>(p);
  return hipGetLastError();
}

}  // namespace nrx
