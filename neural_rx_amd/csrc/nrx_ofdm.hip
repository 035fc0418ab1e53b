// nrx_ofdm.hip -- OFDM modulation and demodulation on the GPU (include/nrx.h "OFDM modulation"), and the
// slot generator's time-domain transmit stage built from them (nrx_generate_slots_td).  tests/ofdm_ref.py
// states the same functions in numpy.
//
//   k_ofdm<R, MOD, NB>  one launch per call.  A (slot, stream, symbol) transform of N = 64..4096 points lives
//                   in LDS from its one global read to its one global write:
//                     modulate    load: grid subcarrier f -> FFT bin (f + first_bin - N/2) mod N, zeros in the
//                                 guard bins, either grid layout; unitary IDFT; store: the last cp samples, then
//                                 the N samples, through the Rapp curve, contiguous in the sample row; the
//                                 workgroup of the last symbol zeroes the row's tail
//                     demodulate  load: the window of N samples (zeros outside the row); unitary DFT; store:
//                                 bin -> subcarrier, the timing-advance ramp e^{+j 2 pi k ta / N}, either layout
//   k_td_h_phase    nrx_gen_td.h_with_delay: h *= e^{-j 2 pi delay k_f / N}, in place on the f32 h
//
// The FFT.  Stockham autosort passes of radix 4 (a radix-2 tail for odd log2 N) in one padded LDS buffer per
// transform: every thread reads the 4 NB inputs of its NB butterflies into registers, a barrier, then writes
// them to their sorted places, a barrier.  N / (4 NB) threads work on a transform, NB = 1 up to N = 1024, 2
// at 2048, 4 at 4096, so that a workgroup is 256 threads and holds 1024 / N transforms for N <= 512 (16 at
// N = 64).  Element i lies at i + (i >> s) with 2^s elements = 256 bytes = one row of the 64 banks, so the
// power-of-two strides of the sorted writes rotate through the banks.
//
// Twiddles.  A workgroup builds the quarter wave e^{-j 2 pi m / N}, m = 0..N/4, once into LDS: f64 sincospi on
// the first octant (N / 8 + 1 evaluations per workgroup, the second octant by the mirror cos <-> sin), rounded
// once to the working precision; the other three quadrants are sign changes and swaps at the lookup.  The
// arguments 2 m / N are exact, so no twiddle carries an argument-reduction error, whatever N.
//
// No atomics, no workspace; every output element has one writer and a fixed operation order, so the bits do
// not depend on the call or on how the batch is split.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nrx.h"
#include "nrx_internal.h"

namespace nrx {

namespace {

constexpr int kFftThreads = 256;

template <class R>
struct alignas(2 * sizeof(R)) Cx {
  R x, y;
};
template <class R>
__device__ __forceinline__ Cx<R> operator+(Cx<R> a, Cx<R> b) { return Cx<R>{a.x + b.x, a.y + b.y}; }
template <class R>
__device__ __forceinline__ Cx<R> operator-(Cx<R> a, Cx<R> b) { return Cx<R>{a.x - b.x, a.y - b.y}; }
template <class R>
__device__ __forceinline__ Cx<R> operator*(Cx<R> a, Cx<R> b) {
  return Cx<R>{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}

// 2^shift elements fill the 64 banks once
template <class R>
__host__ __device__ constexpr int pad_shift() { return sizeof(R) == 4 ? 5 : 4; }
template <class R>
__host__ __device__ constexpr int padded(int i) { return i + (i >> pad_shift<R>()); }

struct OfdmArgs {
  int B, S, F, T, N, first_bin, layout, ta;
  int cp[kT];
  int start[kT];       // first sample of symbol t in the row: sum over t' < t of cp[t'] + N
  int offset[16];
  long long L, total;  // samples per row; transforms B S T
  int pa_on;
  double pa_inv_a2, pa_p;
  void* grid;
  void* samples;
};

// e^{-j 2 pi m / N} (CONJ: e^{+j ...}), 0 <= m < N, from the quarter wave tw[0..N/4]
template <class R, bool CONJ>
__device__ __forceinline__ Cx<R> twiddle(const Cx<R>* tw, int m, int l4) {
  const int q = m >> l4, i = m & ((1 << l4) - 1);      // l4 = log2(N / 4)
  const Cx<R> w = tw[i];
  Cx<R> r;
  r.x = q == 0 ? w.x : (q == 1 ? w.y : (q == 2 ? -w.x : -w.y));
  r.y = q == 0 ? w.y : (q == 1 ? -w.x : (q == 2 ? -w.y : w.x));
  if (CONJ) r.y = -r.y;
  return r;
}

template <class R>
__device__ __forceinline__ Cx<R> load_grid(const OfdmArgs& a, long long b, int s, int f, int t) {
  if (a.layout == NRX_OFDM_GRID_PLANAR)
    return reinterpret_cast<const Cx<R>*>(a.grid)[((b * a.S + s) * a.F + f) * a.T + t];
  const R* g = reinterpret_cast<const R*>(a.grid) + ((b * a.F + f) * a.T + t) * 2 * a.S;
  return Cx<R>{g[s], g[a.S + s]};
}

template <class R>
__device__ __forceinline__ void store_grid(const OfdmArgs& a, long long b, int s, int f, int t, Cx<R> v) {
  if (a.layout == NRX_OFDM_GRID_PLANAR) {
    reinterpret_cast<Cx<R>*>(a.grid)[((b * a.S + s) * a.F + f) * a.T + t] = v;
    return;
  }
  R* g = reinterpret_cast<R*>(a.grid) + ((b * a.F + f) * a.T + t) * 2 * a.S;
  g[s] = v.x;
  g[a.S + s] = v.y;
}

// Rapp AM/AM curve v / (1 + (|v| / A)^(2p))^(1 / (2p)), in f64 whatever the sample type
template <class R>
__device__ __forceinline__ Cx<R> rapp(Cx<R> v, double inv_a2, double p) {
  const double re = v.x, im = v.y;
  const double g = pow(1.0 + pow((re * re + im * im) * inv_a2, p), -0.5 / p);
  return Cx<R>{(R)(re * g), (R)(im * g)};
}

// The in-LDS transform of `buf` (padded, natural order in and out) by the n / (4 NB) threads `lt` of
// its group; INV: the inverse (conjugate twiddles).  Unscaled.  Every thread of the workgroup calls it:
// the barriers are the workgroup's.
template <class R, bool INV, int NB>
__device__ __forceinline__ void fft_lds(Cx<R>* buf, const Cx<R>* tw, int n, int lt) {
  const int tpt = n / (4 * NB), n4 = n >> 2, l4 = 31 - __clz(n4);
  int ns = 1;
  for (; ns * 4 <= n; ns *= 4) {
    Cx<R> v[NB][4];
    const int stride = n4 / ns;                // N / (4 Ns)
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int j = lt + i * tpt, k = j & (ns - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[i][r] = buf[padded<R>(j + r * n4)];
      if (ns > 1) {
        const int m = k * stride;
        v[i][1] = v[i][1] * twiddle<R, INV>(tw, m, l4);
        v[i][2] = v[i][2] * twiddle<R, INV>(tw, 2 * m, l4);
        v[i][3] = v[i][3] * twiddle<R, INV>(tw, 3 * m, l4);
      }
      const Cx<R> t0 = v[i][0] + v[i][2], t1 = v[i][0] - v[i][2], t2 = v[i][1] + v[i][3], d = v[i][1] - v[i][3];
      const Cx<R> t3 = INV ? Cx<R>{-d.y, d.x} : Cx<R>{d.y, -d.x};      // +-j (v1 - v3)
      v[i][0] = t0 + t2;
      v[i][1] = t1 + t3;
      v[i][2] = t0 - t2;
      v[i][3] = t1 - t3;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int j = lt + i * tpt, k = j & (ns - 1);
      const int base = ((j - k) << 2) + k;
#pragma unroll
      for (int r = 0; r < 4; ++r) buf[padded<R>(base + r * ns)] = v[i][r];
    }
    __syncthreads();
  }
  if (ns < n) {        // radix-2 tail, Ns = N / 2: butterfly j reads and writes the places j and j + N / 2
#pragma unroll
    for (int i = 0; i < 2 * NB; ++i) {
      const int j = lt + i * tpt;
      const Cx<R> p = buf[padded<R>(j)], q = buf[padded<R>(j + ns)] * twiddle<R, INV>(tw, j, l4);
      buf[padded<R>(j)] = p + q;
      buf[padded<R>(j + ns)] = p - q;
    }
    __syncthreads();
  }
}

// grid ceil(B S T / G), G = 256 / (N / (4 NB)) transforms per workgroup; transform g = (b S + s) T + t.
// Dynamic LDS: the quarter wave [N / 4 + 1], then G padded buffers.
template <class R, bool MOD, int NB>
__global__ __launch_bounds__(kFftThreads) void k_ofdm(OfdmArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  using C = Cx<R>;
  const int N = a.N, n4 = N >> 2;
  const int tpt = N / (4 * NB);
  const int G = kFftThreads / tpt;
  const int tid = threadIdx.x, tl = tid / tpt, lt = tid - tl * tpt;
  C* tw = reinterpret_cast<C*>(smem);
  C* buf = tw + (n4 + 1) + (size_t)tl * padded<R>(N);

  for (int m = tid; m <= N / 8; m += kFftThreads) {
    double s, c;
    sincospi(2.0 * m / N, &s, &c);
    tw[m] = C{(R)c, (R)-s};
    tw[n4 - m] = C{(R)s, (R)-c};
  }

  const long long g = (long long)blockIdx.x * G + tl;
  const bool valid = g < a.total;          // uniform over the transform's threads
  const int t = (int)(g % a.T);
  const int s = (int)((g / a.T) % a.S);
  const long long b = g / ((long long)a.T * a.S);
  const long long row = (b * a.S + s) * a.L;
  const int fb = a.first_bin;
  C* smp = reinterpret_cast<C*>(a.samples);

  if (MOD) {
    for (int k = lt; k < N; k += tpt) {
      const int f = ((k + (N >> 1)) & (N - 1)) - fb;
      C v{(R)0, (R)0};
      if (valid && f >= 0 && f < a.F) v = load_grid<R>(a, b, s, f, t);
      buf[padded<R>(k)] = v;
    }
  } else {
    const long long w0 = valid ? (long long)a.offset[s] + a.start[t] + a.cp[t] - a.ta : 0;
    for (int n = lt; n < N; n += tpt) {
      const long long p = w0 + n;
      C v{(R)0, (R)0};
      if (valid && p >= 0 && p < a.L) v = smp[row + p];
      buf[padded<R>(n)] = v;
    }
  }
  __syncthreads();
  fft_lds<R, MOD, NB>(buf, tw, N, lt);
  if (!valid) return;
  const R scale = (R)(1.0 / sqrt((double)N));
  if (MOD) {
    const int cp = a.cp[t], len = cp + N;
    C* dst = smp + row + a.start[t];
    for (int i = lt; i < len; i += tpt) {
      C v = buf[padded<R>((i + N - cp) & (N - 1))];
      v.x *= scale;
      v.y *= scale;
      if (a.pa_on) v = rapp<R>(v, a.pa_inv_a2, a.pa_p);
      dst[i] = v;
    }
    if (t == a.T - 1)
      for (long long i = (long long)a.start[t] + len + lt; i < a.L; i += tpt) smp[row + i] = C{(R)0, (R)0};
  } else {
    for (int f = lt; f < a.F; f += tpt) {
      const int k = (f + fb + (N >> 1)) & (N - 1);
      C v = buf[padded<R>(k)];
      v.x *= scale;
      v.y *= scale;
      if (a.ta) v = v * twiddle<R, true>(tw, (k * a.ta) & (N - 1), 31 - __clz(n4));
      store_grid<R>(a, b, s, f, t, v);
    }
  }
}

template <class R, bool MOD, int NB>
hipError_t launch_k(const OfdmArgs& a, hipStream_t st) {
  const int tpt = a.N / (4 * NB), G = kFftThreads / tpt;
  const size_t lds = ((size_t)(a.N / 4 + 1) + (size_t)G * padded<R>(a.N)) * sizeof(Cx<R>);
  if (lds > 64 * 1024)
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ofdm<R, MOD, NB>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
      return e;
  k_ofdm<R, MOD, NB><<<(unsigned)((a.total + G - 1) / G), kFftThreads, lds, st>>>(a);
  return hipGetLastError();
}

template <class R, bool MOD>
hipError_t launch_n(const OfdmArgs& a, hipStream_t st) {
  if (a.N <= 1024) return launch_k<R, MOD, 1>(a, st);
  if (a.N == 2048) return launch_k<R, MOD, 2>(a, st);
  return launch_k<R, MOD, 4>(a, st);
}

// one thread per complex element (b, u, f, t, a) of h [B][U][F][14][2A]; f64 arithmetic, one f32 rounding
__global__ __launch_bounds__(256) void k_td_h_phase(nrx_gen_desc d, nrx_gen_td td, int first_bin,
                                                    float* __restrict__ h) {
  const int U = d.num_tx, F = d.num_subcarriers, A = d.num_rx_ant, N = td.fft_size;
  const int64_t n = (int64_t)d.batch * U * F * kT * A;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int ant = (int)(i % A);
  const int64_t r = i / A;                 // (b, u, f, t)
  const int f = (int)((r / kT) % F);
  const int u = (int)((r / ((int64_t)kT * F)) % U);
  const int kf = f + first_bin - (N >> 1);
  const long long m = (((long long)td.delay[u] * kf) % N + N) % N;
  double sn, cs;
  sincospi(-2.0 * (double)m / N, &sn, &cs);
  float* p = h + r * 2 * A + ant;
  const double hr = p[0], hi = p[A];
  p[0] = (float)(hr * cs - hi * sn);
  p[A] = (float)(hr * sn + hi * cs);
}

int resolve_first_bin(int first_bin, int N, int F) { return first_bin < 0 ? N / 2 - F / 2 : first_bin; }

}  // namespace

hipError_t launch_ofdm(const nrx_ofdm_io& io, bool modulate, hipStream_t st) {
  OfdmArgs a{};
  a.B = io.batch, a.S = io.num_streams, a.F = io.grid_subcarriers, a.T = io.num_symbols, a.N = io.fft_size;
  a.first_bin = resolve_first_bin(io.first_bin, a.N, a.F);
  a.layout = io.grid_layout;
  a.ta = modulate ? 0 : io.timing_advance;
  int at = 0;
  for (int t = 0; t < a.T; ++t) {
    a.cp[t] = io.cp_length[t];
    a.start[t] = at;
    at += a.cp[t] + a.N;
  }
  for (int s = 0; s < a.S; ++s) a.offset[s] = modulate ? 0 : io.offset[s];
  a.L = io.num_samples;
  a.total = (long long)a.B * a.S * a.T;
  a.pa_on = modulate && io.pa_asat > 0.0;
  if (a.pa_on) {
    a.pa_inv_a2 = 1.0 / (io.pa_asat * io.pa_asat);
    a.pa_p = io.pa_smoothness;
  }
  a.grid = io.grid, a.samples = io.samples;
  if (io.precision == NRX_OFDM_F32) return modulate ? launch_n<float, true>(a, st) : launch_n<float, false>(a, st);
  return modulate ? launch_n<double, true>(a, st) : launch_n<double, false>(a, st);
}

// ---- the generator's time-domain stage: x' = demodulate(impair(modulate(x))) per (slot, port), f64

struct TdWs {
  double2* xp;        // [B][U][F][14]
  double2* samples;   // [B][U][Ls]
};

static size_t td_layout(const nrx_gen_desc& d, const nrx_gen_td& td, TdWs* w, void* base) {
  Carver c(base);
  TdWs v;
  v.xp = c.take<double2>(gen_grid_elems(d));
  v.samples = c.take<double2>((size_t)d.batch * d.num_tx * (size_t)slot_samples(td.cp_length, td.fft_size, kT));
  if (w) *w = v;
  return c.bytes();
}

size_t td_workspace_bytes(const nrx_gen_desc& d, const nrx_gen_td& td) { return td_layout(d, td, nullptr, nullptr); }

hipError_t launch_td_apply(const nrx_gen_desc& d, const nrx_gen_td& td, const double* x, void* ws, hipStream_t st) {
  TdWs w;
  td_layout(d, td, &w, ws);
  nrx_ofdm_io io = stage_ofdm(d, td, d.num_tx, const_cast<double*>(x), w.samples);
  if (td.pa_enable) {
    io.pa_asat = sqrt((double)d.num_subcarriers / td.fft_size) * pow(10.0, td.pa_ibo_db / 20.0);
    io.pa_smoothness = td.pa_smoothness;
  }
  if (hipError_t e = launch_ofdm(io, /*modulate=*/true, st)) return e;
  for (int u = 0; u < d.num_tx; ++u) io.offset[u] = -td.delay[u];
  io.grid = w.xp;
  if (hipError_t e = launch_ofdm(io, /*modulate=*/false, st)) return e;
  if (td.x_out)
    return hipMemcpyAsync(td.x_out, w.xp, gen_grid_elems(d) * sizeof(double2), hipMemcpyDeviceToDevice, st);
  return hipSuccess;
}

hipError_t launch_td_h_phase(const nrx_gen_desc& d, const nrx_gen_td& td, float* h, hipStream_t st) {
  const int64_t n = (int64_t)d.batch * d.num_tx * d.num_subcarriers * kT * d.num_rx_ant;
  k_td_h_phase<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(
      d, td, resolve_first_bin(td.first_bin, td.fft_size, d.num_subcarriers), h);
  return hipGetLastError();
}

}  // namespace nrx
