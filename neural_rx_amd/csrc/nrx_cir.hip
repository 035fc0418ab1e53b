// nrx_cir.hip -- the slot generator on caller-supplied channel impulse responses (include/nrx.h
// "channel impulse response replay"; tests/cir_ref.py states the same function in numpy f64).
//
//   k_cir_h       per (slot, user): H[f][a, t] = sum_l E[f][l] G[l][a, t], a complex F x L by L x 14A
//                 product on v_mfma_f64_16x16x4_f64.  A workgroup owns one (slot, user), kCirTM
//                 subcarriers (one 16-row tile per wave) and up to kCirTN of the 14A columns padded to
//                 a multiple of 16: M = subcarriers, N = (antenna, symbol) columns, K = paths.  The
//                 paths are walked in chunks of kCirKC through LDS: the phasors E of the chunk are
//                 made once per (tile, path) -- one sincos at the first row of each half tile and one
//                 of the subcarrier step, then seven complex multiplications down the rows -- and are
//                 shared by every antenna and symbol; the coefficients G are widened from f32 into a
//                 real and an imaginary plane.  Four real MFMAs per complex step.  H goes to the
//                 workspace in f64 and the energy of the workgroup's elements to a slot of its own.
//   k_cir_scale   per (slot, user): the energy slots summed in index order, 1 / sqrt(mean |H|^2)
//   k_cir_rx      per (slot, subcarrier): y[a][t] = sum_u s_u H_u x_u + AWGN and the true channel, the
//                 arithmetic, noise indices and stores of k_gen_rx (nrx_synth.hip) on the replayed H
//
// No atomics: every output element and every energy slot has one writer, and every sum a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nrx.h"
#include "nrx_internal.h"
#include "nrx_rng.h"

namespace nrx {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kCirTM = 64;        // subcarriers of a workgroup: four waves, a 16-row tile each
constexpr int kCirTN = 64;        // columns (antenna, symbol) of a workgroup: four 16-column tiles
constexpr int kCirKC = 32;        // paths staged per chunk
constexpr int kCirThreads = 256;

struct CirWs {
  double2* H;      // [B][U][F][14 A], column a 14 + t
  double* part;    // [B][U][F tiles][column groups]: sum |H|^2 of one k_cir_h workgroup
  double* scale;   // [B][U]
};

__host__ __device__ inline int cir_cols_padded(int A) { return (kT * A + 15) / 16 * 16; }
__host__ __device__ inline int cir_col_groups(int A) { return (cir_cols_padded(A) + kCirTN - 1) / kCirTN; }
__host__ __device__ inline int cir_f_tiles(int F) { return (F + kCirTM - 1) / kCirTM; }
// row stride of the coefficient planes in doubles: 16 modulo 32, so that the four rows a wave reads in
// one step start 128 bytes apart modulo the 256 bytes of the LDS banks
__host__ __device__ inline int cir_g_stride(int ncol) { return ncol % 32 == 16 ? ncol : ncol + 16; }

size_t cir_ws(const nrx_gen_desc& d, CirWs* w, void* base) {
  const size_t BU = (size_t)d.batch * d.num_tx, F = d.num_subcarriers, A = d.num_rx_ant;
  Carver c(base);
  CirWs v;
  v.H = c.take<double2>(BU * F * kT * A);
  v.part = c.take<double>(BU * cir_f_tiles((int)F) * cir_col_groups((int)A));
  v.scale = c.take<double>(BU);
  if (w) *w = v;
  return c.bytes();
}

// the example of (slot b, user u), or -1: a zero channel
__device__ __forceinline__ int cir_example(const nrx_gen_desc& d, const nrx_gen_cir& c, int64_t b, int u) {
  const int E = c.num_examples, U = d.num_tx;
  int64_t e;
  if (c.select == 0) {
    e = c.index[b * U + u];
  } else {
    const uint32_t w = draw(d, b, ST_CIR, (uint32_t)u).x;
    e = c.select == 1 ? (int64_t)(w % (uint32_t)E) : (int64_t)U * (w % (uint32_t)(E / U)) + u;
  }
  return e >= 0 && e < E ? (int)e : -1;
}

// grid (B * U, F tiles, column groups); dynamic LDS: the phasors [4][kCirKC][16] complex, then the two
// coefficient planes [kCirKC][stride]
__global__ __launch_bounds__(kCirThreads) void k_cir_h(nrx_gen_desc d, nrx_gen_cir c, CirWs w) {
  extern __shared__ double2 smem[];
  __shared__ double red[4];
  const int F = d.num_subcarriers, U = d.num_tx, A = d.num_rx_ant, L = c.num_paths, Ta = c.num_time_steps;
  const int NC = kT * A;
  const int64_t bu = blockIdx.x;
  const int64_t b = bu / U;
  const int u = (int)(bu % U);
  const int k0 = blockIdx.y * kCirTM;
  const int c0 = blockIdx.z * kCirTN;
  const int ncol = cir_cols_padded(A) - c0 < kCirTN ? cir_cols_padded(A) - c0 : kCirTN;   // multiple of 16
  const int nct = ncol >> 4;
  const int S = cir_g_stride(ncol);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kk = lane >> 4;
  double2* Hb = w.H + (size_t)bu * F * NC;
  double* part = w.part + ((size_t)bu * gridDim.y + blockIdx.y) * gridDim.z + blockIdx.z;
  const int nrows = F - k0 < kCirTM ? F - k0 : kCirTM;
  const int ncv = NC - c0 < ncol ? NC - c0 : ncol;          // columns of this group that exist
  const int e = cir_example(d, c, b, u);
  if (e < 0) {                                              // uniform: a zero channel, nothing of the dataset is read
    for (int i = tid; i < nrows * ncv; i += kCirThreads)
      Hb[(size_t)(k0 + i / ncv) * NC + c0 + i % ncv] = make_double2(0.0, 0.0);
    if (tid == 0) *part = 0.0;
    return;
  }
  double2* es = smem;
  double* g_re = reinterpret_cast<double*>(smem + 4 * kCirKC * 16);
  double* g_im = g_re + kCirKC * S;
  const float2* ae = reinterpret_cast<const float2*>(c.a) + (size_t)e * A * L * Ta;
  const float* te = c.tau + (size_t)e * L;
  // the padded columns stay zero: the chunks below write the existing ones only
  for (int i = tid; i < 2 * kCirKC * S; i += kCirThreads) g_re[i] = 0.0;
  const int a_lo = c0 / kT;
  const int a_hi = (c0 + ncv - 1) / kT;                     // < A
  const int na = a_hi - a_lo + 1;
  const bool tile = k0 + 16 * wave < F;                     // uniform over the wave
  f64x4 accr[4], acci[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) accr[ct] = acci[ct] = f64x4{0.0, 0.0, 0.0, 0.0};

  for (int l0 = 0; l0 < L; l0 += kCirKC) {
    __syncthreads();                                        // the planes are zeroed; the previous chunk has been read
    {  // phasors: thread (tile, path, half) walks 8 subcarriers from f0 = k0 + 16 tile + 8 half
      const int half = tid & 1, p = (tid >> 1) % kCirKC, tl = tid / (2 * kCirKC);
      double2* dst = es + ((size_t)(tl * kCirKC + p) * 16 + 8 * half);
      const int l = l0 + p;
      if (l < L) {
        const double tau = (double)te[l];
        const double f0 = (double)(k0 + 16 * tl + 8 * half) + c.f_offset;
        double s0, c0r, s1, c1;
        sincos(2.0 * kPi * ((f0 * d.subcarrier_spacing) * tau), &s0, &c0r);
        sincos(2.0 * kPi * (d.subcarrier_spacing * tau), &s1, &c1);
        double er = c0r, ei = -s0;                          // e^{-j phi}
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          dst[i] = make_double2(er, ei);
          const double nr = er * c1 + ei * s1, ni = ei * c1 - er * s1;     // times e^{-j step}
          er = nr;
          ei = ni;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[i] = make_double2(0.0, 0.0);
      }
    }
    if (Ta == 1) {                                          // one load per (antenna, path), 14 columns written
      for (int i = tid; i < na * kCirKC; i += kCirThreads) {
        const int a = a_lo + i / kCirKC, p = i % kCirKC, l = l0 + p;
        float2 v = make_float2(0.0f, 0.0f);
        if (l < L) v = ae[(size_t)a * L + l];
        for (int t = 0; t < kT; ++t) {
          const int cl = a * kT + t - c0;
          if (cl >= 0 && cl < ncv) {
            g_re[p * S + cl] = (double)v.x;
            g_im[p * S + cl] = (double)v.y;
          }
        }
      }
    } else {                                                // [path][symbol] of one antenna is contiguous
      for (int i = tid; i < na * kCirKC * kT; i += kCirThreads) {
        const int a = a_lo + i / (kCirKC * kT), r = i % (kCirKC * kT);
        const int p = r / kT, t = r % kT, l = l0 + p;
        const int cl = a * kT + t - c0;
        if (cl < 0 || cl >= ncv) continue;
        float2 v = make_float2(0.0f, 0.0f);
        if (l < L) v = ae[((size_t)a * L + l) * kT + t];
        g_re[p * S + cl] = (double)v.x;
        g_im[p * S + cl] = (double)v.y;
      }
    }
    __syncthreads();
    if (tile) {
      const int steps = L - l0 < kCirKC ? (L - l0 + 3) >> 2 : kCirKC / 4;
      for (int s = 0; s < steps; ++s) {
        const double2 ev = es[(size_t)(wave * kCirKC + 4 * s + kk) * 16 + col];   // A operand: row = lane & 15
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          if (ct < nct) {
            const double gr = g_re[(4 * s + kk) * S + 16 * ct + col], gi = g_im[(4 * s + kk) * S + 16 * ct + col];
            accr[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ev.x, gr, accr[ct], 0, 0, 0);
            acci[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ev.x, gi, acci[ct], 0, 0, 0);
            accr[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ev.y, -gi, accr[ct], 0, 0, 0);
            acci[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ev.y, gr, acci[ct], 0, 0, 0);
          }
        }
      }
    }
  }
  // C / D layout of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 register
  double en = 0.0;
  if (tile) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      if (ct < nct && 16 * ct + col < ncv) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = k0 + 16 * wave + kk + 4 * r;
          if (f < F) {
            Hb[(size_t)f * NC + c0 + 16 * ct + col] = make_double2(accr[ct][r], acci[ct][r]);
            en += accr[ct][r] * accr[ct][r] + acci[ct][r] * acci[ct][r];
          }
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) en += __shfl_xor(en, o);
  if (lane == 0) red[wave] = en;
  __syncthreads();
  if (tid == 0) *part = ((red[0] + red[1]) + red[2]) + red[3];
}

// one thread per (slot, user): its energy slots in index order
__global__ __launch_bounds__(64) void k_cir_scale(CirWs w, int64_t nbu, int nparts, double count) {
  const int64_t bu = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (bu >= nbu) return;
  double s = 0.0;
  for (int i = 0; i < nparts; ++i) s += w.part[bu * nparts + i];
  const double cm = s / count;
  w.scale[bu] = cm > 0.0 ? 1.0 / sqrt(cm) : 0.0;
}

// block = FB subcarriers x (A * T) threads; grid = (ceil(F / FB), B): k_gen_rx on the replayed channel
__global__ __launch_bounds__(256) void k_cir_rx(nrx_gen_desc d, CirWs w, int normalize, const double2* __restrict__ x,
                                                const double* __restrict__ no_slot, int FB, float* __restrict__ y, float* __restrict__ h,
                                                float* __restrict__ y_re, float* __restrict__ y_im) {
  const int U = d.num_tx, A = d.num_rx_ant, F = d.num_subcarriers, T = d.num_symbols;
  const int b = blockIdx.y;
  const int fl = threadIdx.x / (A * T);
  const int f = blockIdx.x * FB + fl;
  if (fl >= FB || f >= F) return;
  const int at = threadIdx.x % (A * T);
  const int a = at / T, t = at % T;
  double yr = 0.0, yi = 0.0;
  for (int u = 0; u < U; ++u) {
    const size_t bu = (size_t)b * U + u;
    double2 hv = w.H[(bu * F + f) * (size_t)(A * T) + at];
    if (normalize) {
      const double s = w.scale[bu];
      hv.x *= s;
      hv.y *= s;
    }
    const double hr = hv.x, hi = hv.y;
    const double2 xv = x[((bu * F) + f) * T + t];
    yr += hr * xv.x - hi * xv.y;
    yi += hr * xv.y + hi * xv.x;
    if (h) {
      float* dst = h + (((bu * F) + f) * T + t) * 2 * A;
      dst[a] = (float)hr;
      dst[A + a] = (float)hi;
    }
  }
  const U4 r = draw(d, b, ST_NOISE, (uint32_t)((a * F + f) * T + t));
  const double2 z = box_muller(r.x, r.y);
  const double sd = sqrt((no_slot ? no_slot[b] : d.no) / 2.0);
  yr += sd * z.x;
  yi += sd * z.y;
  const size_t ft = ((size_t)b * F + f) * T + t;
  y[ft * 2 * A + a] = (float)yr;
  y[ft * 2 * A + A + a] = (float)yi;
  if (y_re) {
    y_re[ft * A + a] = (float)yr;
    y_im[ft * A + a] = (float)yi;
  }
}

}  // namespace

size_t cir_workspace_bytes(const nrx_gen_desc& d) { return cir_ws(d, nullptr, nullptr); }

hipError_t launch_cir_rx(const nrx_gen_desc& d, const nrx_gen_cir& c, const double* x, void* ws,
                         const double* no_slot, float* y, float* h, float* y_re, float* y_im, hipStream_t st) {
  CirWs w;
  cir_ws(d, &w, ws);
  const int F = d.num_subcarriers, A = d.num_rx_ant;
  const int64_t BU = (int64_t)d.batch * d.num_tx;
  const int nft = cir_f_tiles(F), ncg = cir_col_groups(A);
  const int ncol = cir_cols_padded(A) < kCirTN ? cir_cols_padded(A) : kCirTN;
  const size_t lds = (size_t)4 * kCirKC * 16 * sizeof(double2) + (size_t)2 * kCirKC * cir_g_stride(ncol) * sizeof(double);
  k_cir_h<<<dim3((unsigned)BU, (unsigned)nft, (unsigned)ncg), kCirThreads, lds, st>>>(d, c, w);
  if (c.normalize)
    k_cir_scale<<<(unsigned)((BU + 63) / 64), 64, 0, st>>>(w, BU, nft * ncg, (double)A * F * kT);
  const int at = A * kT;
  int FB = 256 / at;
  if (FB > 4) FB = 4;
  k_cir_rx<<<dim3((unsigned)((F + FB - 1) / FB), (unsigned)d.batch), FB * at, 0, st>>>(
      d, w, c.normalize, reinterpret_cast<const double2*>(x), no_slot, FB, y, h, y_re, y_im);
  return hipGetLastError();
}

}  // namespace nrx
