// nrx_ldpc.hip -- layered belief-propagation decoder of a quasi-cyclic LDPC code and the slot glue
// of a coded evaluation (include/nrx.h: nrx_ldpc_decode, nrx_ldpc_gather, nrx_ldpc_count).
//
// k_ldpc_decode: one launch runs every iteration.  A workgroup owns G = max(1, 256 / z) codewords
// and has one thread per (codeword g, check r of a layer): thread g z + r.  APP of the G codewords
// lives in LDS; the check-to-variable messages, [g][edge of the base graph][r], live in LDS behind
// it when they fit and in the workspace otherwise.  A message is only ever touched by its own
// thread, so only APP needs the barrier that separates two layers.  A layer's z checks touch
// disjoint variables, a rotated contiguous run per base column, so the LDS accesses of a wave are
// free of bank conflicts.  A check is walked twice without holding its edges in registers: the
// forward walk leaves t_k in the APP slot and the prefix P_{k-1} in the message slot, the backward
// walk carries the suffix and writes the new message and APP.  The stop flags of the codewords and
// of the workgroup are plain LDS words, double-buffered by iteration parity; every thread reaches
// every barrier and the exit is uniform.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nrx.h"
#include "nrx_internal.h"

namespace nrx {

namespace {

constexpr int kLdpcLanes = 256;      // checks a workgroup runs side by side when z is small
constexpr int kLdpcMaxThreads = 384; // z <= 384: one thread per check
constexpr int kLdpcMaxG = kLdpcLanes / 2;
constexpr int kLdpcLdsBudget = 160 * 1024 - 4096;   // dynamic LDS of a workgroup (flags are static)

struct LdpcArgs {
  int mb, nb, z, N, E, G;
  int num_cw, num_iter, cn_type, early_stop;
  float ms_scale, clip;
  const int* row_ptr;                // [mb + 1]
  const int2* edges;                 // [E]: (base column * z, shift), rows in order, columns ascending
  const float* llr_in;
  const uint8_t* skip;
  uint8_t* hard;
  float* app;
  int* iters;
  uint8_t* parity_ok;
  float* ws;                         // messages [num_cw][E][z] when they are not in LDS
};

__device__ __forceinline__ float clampf(float x, float c) { return fminf(fmaxf(x, -c), c); }

__device__ __forceinline__ float boxplus(float a, float b) {
  const float mn = fminf(fabsf(a), fabsf(b));
  const float sg = (a == 0.0f || b == 0.0f) ? 0.0f : ((a < 0.0f) != (b < 0.0f) ? -mn : mn);
  return sg + (log1pf(expf(-fabsf(a + b))) - log1pf(expf(-fabsf(a - b))));   // exactly odd in a and in b
}

template <bool MSG_LDS>
__global__ __launch_bounds__(kLdpcMaxThreads) void k_ldpc_decode(LdpcArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_bad[2][kLdpcMaxG];
  __shared__ int s_more[2];
  const int tid = threadIdx.x, z = p.z, N = p.N;
  const int g = tid / z, r = tid - g * z;
  const int64_t cw = (int64_t)blockIdx.x * p.G + g;
  const bool mine = g < p.G && cw < p.num_cw;
  const bool skipped = mine && p.skip && p.skip[cw];
  bool run = mine && !skipped;                         // uniform over the threads of a codeword
  float* app = reinterpret_cast<float*>(smem) + (mine ? g : 0) * N;
  float* msg;
  if constexpr (MSG_LDS)
    msg = reinterpret_cast<float*>(smem) + p.G * N + (mine ? g : 0) * p.E * z;
  else
    msg = p.ws + (size_t)(mine ? cw : 0) * p.E * z;
  msg += r;                                            // msg[e * z]: edge e of this thread's checks
  const float clip = p.clip;
  if (run) {
    const float* l = p.llr_in + cw * N;
    for (int v = r; v < N; v += z) {
      const float x = l[v];
      app[v] = x != x ? 0.0f : clampf(x, clip);
    }
    for (int e = 0; e < p.E; ++e) msg[e * z] = 0.0f;
  }
  __syncthreads();
  int it = 0;
  bool ok = false;
  for (;;) {
    const int par = it & 1;
    if (tid == 0) s_more[par] = 0;
    if (mine && r == 0) s_bad[par][g] = 0;
    for (int i = 0; i < p.mb; ++i) {
      if (run) {
        const int e0 = p.row_ptr[i], e1 = p.row_ptr[i + 1];
        if (p.cn_type == 0) {
          float P = 0.0f;
          for (int e = e0; e < e1; ++e) {
            const int2 ed = p.edges[e];
            int o = r + ed.y;
            o = o >= z ? o - z : o;
            const float t = app[ed.x + o] - msg[e * z];
            app[ed.x + o] = t;
            msg[e * z] = P;
            P = e == e0 ? t : boxplus(P, t);
          }
          float S = 0.0f;
          for (int e = e1 - 1; e >= e0; --e) {
            const int2 ed = p.edges[e];
            int o = r + ed.y;
            o = o >= z ? o - z : o;
            const float t = app[ed.x + o];
            const float pre = msg[e * z];
            const float x = e == e1 - 1 ? pre : (e == e0 ? S : boxplus(pre, S));
            const float m = clampf(x, clip);
            msg[e * z] = m;
            app[ed.x + o] = t + m;
            S = e == e1 - 1 ? t : boxplus(S, t);
          }
        } else {
          float m1 = INFINITY, m2 = INFINITY;
          int arg = -1;
          bool neg = false;
          for (int e = e0; e < e1; ++e) {
            const int2 ed = p.edges[e];
            int o = r + ed.y;
            o = o >= z ? o - z : o;
            const float t = app[ed.x + o] - msg[e * z];
            app[ed.x + o] = t;
            const float a = fabsf(t);
            neg ^= t < 0.0f;
            if (a < m1) {
              m2 = m1, m1 = a, arg = e;
            } else if (a < m2) {
              m2 = a;
            }
          }
          for (int e = e0; e < e1; ++e) {
            const int2 ed = p.edges[e];
            int o = r + ed.y;
            o = o >= z ? o - z : o;
            const float t = app[ed.x + o];
            const float mag = e == arg ? m2 : m1;
            const float x = p.ms_scale * ((neg != (t < 0.0f)) ? -mag : mag);
            const float m = clampf(x, clip);
            msg[e * z] = m;
            app[ed.x + o] = t + m;
          }
        }
      }
      __syncthreads();                                 // APP of layer i is complete
    }
    ++it;
    const bool last = it >= p.num_iter;
    if (run && (p.early_stop || last)) {
      int bad = 0;
      for (int i = 0; i < p.mb; ++i) {
        int x = 0;
        for (int e = p.row_ptr[i]; e < p.row_ptr[i + 1]; ++e) {
          const int2 ed = p.edges[e];
          int o = r + ed.y;
          o = o >= z ? o - z : o;
          x ^= app[ed.x + o] <= 0.0f ? 1 : 0;
        }
        bad |= x;
      }
      if (bad) s_bad[par][g] = 1;                      // every writer stores the same word
    }
    __syncthreads();
    if (run) {
      ok = (p.early_stop || last) && !s_bad[par][g];
      if (last || (p.early_stop && ok)) {
        run = false;
        if (r == 0) {
          p.iters[cw] = it;
          p.parity_ok[cw] = ok ? 1 : 0;
        }
      } else {
        s_more[par] = 1;
      }
    }
    __syncthreads();
    if (!s_more[par]) break;                           // uniform: no codeword of the workgroup goes on
  }
  if (!mine) return;
  uint8_t* hard = p.hard + cw * N;
  float* out = p.app ? p.app + cw * N : nullptr;
  if (skipped) {
    for (int v = r; v < N; v += z) {
      hard[v] = 0;
      if (out) out[v] = 0.0f;
    }
    if (r == 0) {
      p.iters[cw] = 0;
      p.parity_ok[cw] = 0;
    }
    return;
  }
  for (int v = r; v < N; v += z) {
    const float a = app[v];
    hard[v] = a <= 0.0f ? 1 : 0;
    if (out) out[v] = a;
  }
}

// ------------------------------------------------------------------ slot glue
struct GatherArgs {
  nrx_ldpc_gather_io io;
  int ndsym;
  int dsym[kT];                      // the data symbols, ascending
};

constexpr int kGatherBlock = 256;

// workgroup = codeword (b, u, j).  The row is initialised to col_prior, then the transmitted bits
// are added in chunks of 256 consecutive e'.  With a tx_col, lanes of a chunk may name the same
// column: a lane counts the lower lanes of the chunk with its column (its rank), and round n adds
// the terms of rank n, so a column receives its terms in ascending e'.  No atomics.
__global__ __launch_bounds__(kGatherBlock) void k_ldpc_gather(GatherArgs a) {
  __shared__ int s_col[kGatherBlock];
  const nrx_ldpc_gather_io& c = a.io;
  const int tid = threadIdx.x, N = c.n, C = c.num_cw_per_user;
  const int64_t cw = blockIdx.x;
  const int64_t bu = cw / C;
  const int j = (int)(cw - bu * C);
  float* out = c.llr_in + cw * N;
  bool skip = !(c.active[bu] > 0.0f);
  int m = c.mcs ? c.mcs[bu] : 0;
  m = m < c.num_mcs ? m : c.num_mcs - 1;
  const int nb = c.mcs_bits[m];
  const int F = c.num_subcarriers, BS = c.bits_stride;
  const int64_t nbits = (int64_t)a.ndsym * F * nb;
  if (j >= nbits / c.n_tx) skip = true;
  if (tid == 0) c.skip[cw] = skip ? 1 : 0;
  for (int v = tid; v < N; v += kGatherBlock) out[v] = c.col_prior ? c.col_prior[v] : 0.0f;
  if (skip) return;                                    // uniform
  __syncthreads();
  const int head = c.num_heads > 1 ? m : 0;
  const int64_t grid = (int64_t)F * kT * BS;
  const float* L = c.llr + ((int64_t)head * c.batch * c.num_tx + bu) * grid;
  const uint8_t* cb = c.bits + bu * grid;
  for (int q0 = 0; q0 < c.n_tx; q0 += kGatherBlock) {
    const int q = q0 + tid;
    bool pending = q < c.n_tx;
    float val = 0.0f;
    int col = 0;
    if (pending) {
      const int64_t e = (int64_t)j * c.n_tx + q;
      const int i = (int)(e / nb), k = (int)(e - (int64_t)i * nb);
      const int ts = i / F, f = i - ts * F;
      const int64_t at = ((int64_t)f * kT + a.dsym[ts]) * BS + k;
      const float l = L[at];
      val = cb[at] ? l : -l;
      col = c.tx_col ? c.tx_col[q] : q;
      pending = col >= 0 && col < N;
    }
    if (!c.tx_col) {                                   // distinct columns: uniform branch
      if (pending) out[col] += val;
      continue;
    }
    s_col[tid] = pending ? col : -1;
    __syncthreads();
    int rank = 0;
    if (pending)
      for (int t = 0; t < tid; ++t) rank += s_col[t] == col ? 1 : 0;
    for (int round = 0;; ++round) {
      if (pending && rank == round) {
        out[col] += val;
        pending = false;
      }
      if (!__syncthreads_or(pending)) break;           // also orders the adds of two rounds
    }
  }
}

constexpr int kCountGroups = 32;

// grid (G, U): workgroup (g, u) walks the slots b = g, g + G, ... of user u and their codewords;
// integer sums only, added to the accumulators at the end as in k_count_errors
__global__ __launch_bounds__(256) void k_ldpc_count(nrx_ldpc_count_io c, int G) {
  __shared__ unsigned red[4];
  const int U = c.num_tx, C = c.num_cw_per_user, N = c.n, u = blockIdx.y;
  unsigned long long err_tot = 0, bits_tot = 0, blk_err = 0, blks = 0, it_tot = 0, cws = 0;
  for (int b = blockIdx.x; b < c.batch; b += G) {
    unsigned slot_err = 0, slot_cw = 0;
    for (int j = 0; j < C; ++j) {
      const int64_t cw = ((int64_t)b * U + u) * C + j;
      if (c.skip[cw]) continue;                        // uniform over the workgroup
      const uint8_t* h = c.hard + cw * N;
      unsigned err = 0;
      for (int v = threadIdx.x; v < c.num_info; v += 256) err += h[v] ? 1u : 0u;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) err += __shfl_xor(err, o);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = err;
      __syncthreads();
      slot_err += red[0] + red[1] + red[2] + red[3];
      __syncthreads();
      slot_cw += 1;
      if (c.iters) it_tot += (unsigned)c.iters[cw];
    }
    if (!slot_cw) continue;
    err_tot += slot_err;
    bits_tot += (unsigned long long)slot_cw * c.num_info;
    blk_err += slot_err ? 1 : 0;
    blks += 1;
    cws += slot_cw;
  }
  if (threadIdx.x == 0 && blks) {
    unsigned long long* o = reinterpret_cast<unsigned long long*>(c.counts) + 4 * u;
    atomicAdd(o + 0, err_tot);
    atomicAdd(o + 1, bits_tot);
    atomicAdd(o + 2, blk_err);
    atomicAdd(o + 3, blks);
    if (c.iters && c.iter_counts) {
      unsigned long long* q = reinterpret_cast<unsigned long long*>(c.iter_counts) + 2 * u;
      atomicAdd(q + 0, it_tot);
      atomicAdd(q + 1, cws);
    }
  }
}

}  // namespace

LdpcPlan ldpc_plan(int nb, int z, int num_edges) {
  LdpcPlan pl;
  pl.G = z >= kLdpcLanes ? 1 : kLdpcLanes / z;
  pl.threads = (pl.G * z + 63) / 64 * 64;
  const size_t app = (size_t)pl.G * nb * z * 4, msg = (size_t)pl.G * num_edges * z * 4;
  pl.msg_lds = app + msg <= (size_t)kLdpcLdsBudget;
  pl.lds_bytes = (int)(pl.msg_lds ? app + msg : app);
  return pl;
}

hipError_t ldpc_setup() {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ldpc_decode<true>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLdpcLdsBudget);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ldpc_decode<false>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, kLdpcLdsBudget);
}

hipError_t launch_ldpc_decode(const LdpcDev& d, const nrx_ldpc_io& io, void* ws, hipStream_t st) {
  LdpcArgs p;
  p.mb = d.mb, p.nb = d.nb, p.z = d.z, p.N = d.nb * d.z, p.E = d.num_edges, p.G = d.plan.G;
  p.num_cw = io.num_cw, p.num_iter = io.num_iter, p.cn_type = io.cn_type, p.early_stop = io.early_stop;
  p.ms_scale = io.ms_scale, p.clip = io.llr_clip;
  p.row_ptr = d.row_ptr, p.edges = reinterpret_cast<const int2*>(d.edges);
  p.llr_in = io.llr_in, p.skip = io.skip, p.hard = io.hard, p.app = io.app, p.iters = io.iters;
  p.parity_ok = io.parity_ok, p.ws = (float*)ws;
  const unsigned groups = (unsigned)((io.num_cw + p.G - 1) / p.G);
  if (d.plan.msg_lds)
    k_ldpc_decode<true><<<groups, d.plan.threads, d.plan.lds_bytes, st>>>(p);
  else
    k_ldpc_decode<false><<<groups, d.plan.threads, d.plan.lds_bytes, st>>>(p);
  return hipGetLastError();
}

hipError_t launch_ldpc_gather(const nrx_ldpc_gather_io& io, hipStream_t st) {
  GatherArgs a;
  a.io = io;
  a.ndsym = 0;
  for (int t = 0; t < kT; ++t) {
    a.dsym[t] = 0;
    if (!((io.dmrs_symbol_mask >> t) & 1)) a.dsym[a.ndsym++] = t;
  }
  const unsigned cws = (unsigned)((int64_t)io.batch * io.num_tx * io.num_cw_per_user);
  k_ldpc_gather<<<cws, kGatherBlock, 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_ldpc_count(const nrx_ldpc_count_io& io, hipStream_t st) {
  const int G = io.batch < kCountGroups ? io.batch : kCountGroups;
  k_ldpc_count<<<dim3(G, io.num_tx), 256, 0, st>>>(io, G);
  return hipGetLastError();
}

}  // namespace nrx
