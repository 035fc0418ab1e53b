// nrx_timechan.hip -- the time-domain channel (include/nrx.h "Time-domain channel"): per-sample Doppler and
// fractional-delay taps on the samples between OFDM modulation and demodulation, and the slot generator's
// receive path built on it (nrx_generate_slots_tc).  tests/timechan_ref.py states the same functions in numpy.
//
//   r[b,a,n] = sum_u sum_l g[b,u,a,l](n) v[b,u,l](n)
//   g(n)     = sum_s g0[s] exp(j 2 pi fd[s] (n - n0) / fs)              the sum of sinusoids, per sample
//   v(n)     = sum_{l' = l_min..l_max} sinc(l' - tau fs) x[b,u,n - l']  the fractional-delay FIR, x = 0 outside
//
//   k_timechan<AM, K>  one launch.  A workgroup of 256 threads owns 256 K consecutive samples of one slot and
//                      every antenna of them; thread t owns samples t, t + 256, ..., t + 256 (K - 1) of the tile,
//                      so loads and stores of a wave are contiguous.  Per user the x window (tile + span - 1
//                      samples) goes to LDS once; per (user, path) the span sinc coefficients go to LDS and each
//                      thread forms its K values of v from the window -- once, shared by all antennas -- and
//                      adds g v into K x A register accumulators.
//                      Rotations.  Sample n = tile0 + 16 hi + lo + 256 k (t = 16 hi + lo).  Per (user, path) and
//                      chunk of 4 antennas the workgroup builds, for each of the <= 64 sinusoids, 16 + 16 + 1
//                      exact values (f64 sincospi of the cycle count) in LDS: g0 exp(j th (tile0 - n0 + 16 hi)),
//                      exp(j th lo) and the step exp(j th 256), th = 2 pi fd / fs.  A thread's rotation at its
//                      first sample is one product of two table entries and advances by the step K - 1 times:
//                      (16 + 16 + 1) / 256 sincospi per sinusoid and thread instead of one, and a fixed re-seed
//                      stride of 256 K samples that depends on A alone (K = 4 / 2 / 1 for A <= 4 / 8 / 16, which
//                      keeps 16 complex accumulators), never on the grid or the batch.
//                      rx_mix acts on the finished accumulators; one global read of x per tile (plus the span
//                      overlap), one global write of r.
//   k_tc_draws         the generator's g0 (sqrt(pdp) and the grid-reference phase folded in) and fd of every
//                      sinusoid: the draws of k_gen_taps (nrx_synth.hip), unsummed
//   k_tc_gbar          the window mean of g over the useful part of every symbol, in closed form (Dirichlet)
//   k_tc_h             h = the ISI-free diagonal of the effective channel from the mean taps
//   k_tc_y             y = demodulated grid + the generator's grid noise, f32, CGNN and Aerial layouts
//
// No atomics, no workspace of its own; every output element has one writer and a fixed operation order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nrx.h"
#include "nrx_internal.h"
#include "nrx_rng.h"

namespace nrx {

namespace {

constexpr int kTcThreads = 256;
constexpr int kTcMaxSpan = 256;
constexpr int kTcMaxK = 4;
constexpr int kTcChunk = 4;       // antennas whose sinusoid tables share LDS: at most 4 x 16 sinusoids

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// sinc(v) = sin(pi v) / (pi v), sinc(0) = 1
__device__ __forceinline__ double sinc(double v) { return v == 0.0 ? 1.0 : sinpi(v) / (kPi * v); }

struct TcArgs {
  int B, U, A, L, NS, l_min, l_max;
  long long Ls, n0;
  double fs;
  const double* tau;     // [B][U][L]
  const double2* g0;     // [B][U][A][L][NS]
  const double* fd;      // [B][U][A][L][NS]
  const double2* x;      // [B][U][Ls]
  const double* mix;     // [A][A][2] or null (the generator's is 8-byte aligned: read as doubles)
  double2* r;            // [B][A][Ls]
};

template <int AM, int K>
__global__ __launch_bounds__(kTcThreads) void k_timechan(TcArgs p) {
  constexpr int TILE = kTcThreads * K;
  __shared__ double2 xw[kTcThreads * kTcMaxK + kTcMaxSpan];
  __shared__ double coef[kTcMaxSpan];
  __shared__ double2 ghi[kTcChunk * 16][16];     // g0 exp(j 2 pi fd (tile0 - n0 + 16 hi) / fs)
  __shared__ double2 elo[kTcChunk * 16][16];     // exp(j 2 pi fd lo / fs)
  __shared__ double2 wstep[kTcChunk * 16];       // exp(j 2 pi fd 256 / fs)
  const int t = threadIdx.x;
  const int b = blockIdx.y;
  const long long tile0 = (long long)blockIdx.x * TILE;
  const int U = p.U, A = p.A, L = p.L, NS = p.NS;
  const int span = p.l_max - p.l_min + 1, W = TILE + span - 1;
  double2 acc[K][AM];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int a = 0; a < AM; ++a) acc[k][a] = make_double2(0.0, 0.0);

  for (int u = 0; u < U; ++u) {
    __syncthreads();                       // the previous user's window has been read
    const double2* xr = p.x + ((size_t)b * U + u) * p.Ls;
    for (int i = t; i < W; i += kTcThreads) {
      const long long n = tile0 - p.l_max + i;
      xw[i] = (n >= 0 && n < p.Ls) ? xr[n] : make_double2(0.0, 0.0);
    }
    for (int l = 0; l < L; ++l) {
      double2 v[K];
#pragma unroll
      for (int c = 0; c < AM / kTcChunk; ++c) {
        if (c * kTcChunk >= A) continue;   // uniform over the workgroup
        __syncthreads();                   // window staged; the previous tables and coefficients read
        const int a0 = c * kTcChunk;
        const int nsin = (A - a0 < kTcChunk ? A - a0 : kTcChunk) * NS;
        // sinusoid j of the chunk is (a0 + j / NS, j % NS); its index in g0 / fd:
        auto index = [&](int j) { return ((((size_t)b * U + u) * A + a0 + j / NS) * L + l) * NS + j % NS; };
        if (c == 0 && t < span) coef[t] = sinc((double)(p.l_min + t) - p.tau[((size_t)b * U + u) * L + l] * p.fs);
        for (int e = t; e < nsin * 32; e += kTcThreads) {
          const int j = e >> 5, q = e & 31;
          const size_t i = index(j);
          const double at = q < 16 ? (double)(tile0 - p.n0 + 16 * q) : (double)(q - 16);
          double sn, cs;
          sincospi(2.0 * (p.fd[i] * (at / p.fs)), &sn, &cs);
          if (q < 16) ghi[j][q] = cmul(p.g0[i], make_double2(cs, sn));
          else elo[j][q - 16] = make_double2(cs, sn);
        }
        if (t < nsin) {
          double sn, cs;
          sincospi(2.0 * (p.fd[index(t)] * ((double)kTcThreads / p.fs)), &sn, &cs);
          wstep[t] = make_double2(cs, sn);
        }
        __syncthreads();
        if (c == 0) {
          // taps outermost, the K samples inside: K independent window reads per coefficient, and the unrolled
          // taps keep several LDS reads in flight
#pragma unroll
          for (int k = 0; k < K; ++k) v[k] = make_double2(0.0, 0.0);
          const double2* xp = xw + t + (span - 1);                       // x[n - l_min], walking down to x[n - l_max]
#pragma unroll 4
          for (int j = 0; j < span; ++j) {
            const double cf = coef[j];
#pragma unroll
            for (int k = 0; k < K; ++k) {
              const double2 xx = xp[kTcThreads * k - j];
              v[k].x += cf * xx.x;
              v[k].y += cf * xx.y;
            }
          }
        }
#pragma unroll
        for (int aa = 0; aa < kTcChunk; ++aa) {
          const int a = c * kTcChunk + aa;
          if (a >= A) continue;
          double2 g[K];
#pragma unroll
          for (int k = 0; k < K; ++k) g[k] = make_double2(0.0, 0.0);
#pragma unroll 4
          for (int s = 0; s < NS; ++s) {
            const int j = aa * NS + s;
            double2 z = cmul(ghi[j][t >> 4], elo[j][t & 15]);
            const double2 w = wstep[j];
#pragma unroll
            for (int k = 0; k < K; ++k) {
              g[k].x += z.x;
              g[k].y += z.y;
              if (k + 1 < K) z = cmul(z, w);
            }
          }
#pragma unroll
          for (int k = 0; k < K; ++k) {
            acc[k][a].x += g[k].x * v[k].x - g[k].y * v[k].y;
            acc[k][a].y += g[k].x * v[k].y + g[k].y * v[k].x;
          }
        }
      }
    }
  }

#pragma unroll
  for (int k = 0; k < K; ++k) {
    const long long n = tile0 + t + kTcThreads * k;
    if (n >= p.Ls) continue;
#pragma unroll
    for (int a = 0; a < AM; ++a) {
      if (a >= A) continue;
      double2 o = acc[k][a];
      if (p.mix) {                         // r'[a] = sum_a' M[a][a'] r[a'], a' ascending
        o = make_double2(0.0, 0.0);
#pragma unroll
        for (int a2 = 0; a2 < AM; ++a2) {
          if (a2 >= A) continue;
          const double mr = p.mix[2 * (a * A + a2)], mi = p.mix[2 * (a * A + a2) + 1];
          o.x += mr * acc[k][a2].x - mi * acc[k][a2].y;
          o.y += mr * acc[k][a2].y + mi * acc[k][a2].x;
        }
      }
      p.r[((size_t)b * A + a) * p.Ls + n] = o;
    }
  }
}

template <int AM, int K>
hipError_t launch_tc_k(const TcArgs& p, hipStream_t st) {
  const long long tile = (long long)kTcThreads * K;
  k_timechan<AM, K><<<dim3((unsigned)((p.Ls + tile - 1) / tile), (unsigned)p.B), kTcThreads, 0, st>>>(p);
  return hipGetLastError();
}

hipError_t launch_tc_args(const TcArgs& p, hipStream_t st) {
  if (p.A <= 4) return launch_tc_k<4, 4>(p, st);
  if (p.A <= 8) return launch_tc_k<8, 2>(p, st);
  return launch_tc_k<16, 1>(p, st);
}

// ---- the generator's pieces

struct TcGen {
  int N, F, first_bin, l_min, l_max, ta;
  int wt[kT];            // first sample of the receive window of symbol t: start[t] + cp[t] - ta
  long long Ls, n0;
  double fs;
};

// one thread per sinusoid (b, u, a, l, s): the draws of k_gen_taps, with sqrt(pdp_l) and the phase
// exp(+j 2 pi (first_bin - N/2) scs tau_l) that refers the delay ramp to grid subcarrier 0 folded into g0
__global__ __launch_bounds__(256) void k_tc_draws(nrx_gen_desc d, nrx_gen_chan ch, TcGen tg,
                                                  const double* __restrict__ tau, const double* __restrict__ spdp,
                                                  double2* __restrict__ g0, double* __restrict__ fd) {
  const int U = d.num_tx, A = d.num_rx_ant, L = d.num_taps, NS = d.num_sinusoids;
  const int64_t n = (int64_t)d.batch * U * A * L * NS;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = (int)(i % NS);
  const int l = (int)((i / NS) % L);
  const int a = (int)((i / ((int64_t)NS * L)) % A);
  const int u = (int)((i / ((int64_t)NS * L * A)) % U);
  const int64_t b = i / ((int64_t)NS * L * A * U);
  const U4 r = draw(d, b, ST_TAP, (uint32_t)((((u * A + a) * L + l) * NS) + s));
  const double2 z = box_muller(r.x, r.y);
  const double sc = 1.0 / sqrt(2.0 * NS);
  const size_t bul = ((size_t)b * U + u) * L + l;
  const double sp = spdp[bul];
  const double ph = 2.0 * kPi * (((double)(tg.first_bin - tg.N / 2) * d.subcarrier_spacing) * tau[bul]);
  g0[i] = cmul(make_double2(z.x * sc * sp, z.y * sc * sp), make_double2(cos(ph), sin(ph)));
  fd[i] = ch.max_doppler_hz[u] * cos(2.0 * kPi * uni(r.z));
}

// gbar[b,u,a,l,t] = (1/N) sum_{m<N} g(w_t + m): with q = fd / fs cycles per sample, the mean of a sinusoid
// over the window is exp(j 2 pi q (w_t - n0 + (N-1)/2)) sinpi(N q) / (N sinpi(q)) (1 at q = 0).
// One thread per (b, u, a, l, t); the layout of the generator's taps [B][U][A][L][14].
__global__ __launch_bounds__(256) void k_tc_gbar(TcGen tg, int NS, int64_t n, const double2* __restrict__ g0,
                                                 const double* __restrict__ fd, double2* __restrict__ gt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int t = (int)(i % kT);
  const int64_t g = i / kT;
  const double mid = (double)(tg.wt[t] - tg.n0) + 0.5 * (double)(tg.N - 1);
  double ar = 0.0, ai = 0.0;
  for (int s = 0; s < NS; ++s) {
    const double q = fd[g * NS + s] / tg.fs;
    const double den = sinpi(q);
    const double amp = den == 0.0 ? 1.0 : sinpi((double)tg.N * q) / ((double)tg.N * den);
    double sn, cs;
    sincospi(2.0 * (q * mid), &sn, &cs);
    const double2 z = g0[g * NS + s];
    ar += amp * (z.x * cs - z.y * sn);
    ai += amp * (z.x * sn + z.y * cs);
  }
  gt[i] = make_double2(ar, ai);
}

// h[b,u,f,t,a] = sum_l gbar_t[l] E[l,f], E = sum_l' sinc(l' - tau_l fs) exp(-j 2 pi k_f l' / N), k_f = f +
// first_bin - N/2.  block = FB subcarriers x (A * T) threads, grid (ceil(F / FB), B), as k_gen_rx
__global__ __launch_bounds__(256) void k_tc_h(nrx_gen_desc d, TcGen tg, int FB, const double* __restrict__ tau,
                                              const double2* __restrict__ gt, float* __restrict__ h) {
  __shared__ double2 e[4][kMaxUsers * 8];
  const int U = d.num_tx, A = d.num_rx_ant, L = d.num_taps, F = d.num_subcarriers, T = kT, N = tg.N;
  const int b = blockIdx.y;
  for (int j = threadIdx.x; j < FB * U * L; j += blockDim.x) {
    const int ff = blockIdx.x * FB + j / (U * L);
    const int ul = j % (U * L);
    if (ff < F) {
      const int kf = ff + tg.first_bin - N / 2;
      const double dly = tau[(size_t)b * U * L + ul] * tg.fs;
      double er = 0.0, ei = 0.0;
      for (int lp = tg.l_min; lp <= tg.l_max; ++lp) {
        const long long m = (((long long)kf * lp) % N + N) % N;
        double sn, cs;
        sincospi(-2.0 * (double)m / N, &sn, &cs);
        const double c = sinc((double)lp - dly);
        er += c * cs;
        ei += c * sn;
      }
      e[j / (U * L)][ul] = make_double2(er, ei);
    }
  }
  __syncthreads();
  const int fl = threadIdx.x / (A * T);
  const int f = blockIdx.x * FB + fl;
  if (fl >= FB || f >= F) return;
  const int at = threadIdx.x % (A * T);
  const int a = at / T, t = at % T;
  for (int u = 0; u < U; ++u) {
    const double2* g = gt + ((((size_t)b * U + u) * A + a) * L) * T + t;
    double hr = 0.0, hi = 0.0;
    for (int l = 0; l < L; ++l) {
      const double2 gl = g[(size_t)l * T], el = e[fl][u * L + l];
      hr += gl.x * el.x - gl.y * el.y;
      hi += gl.x * el.y + gl.y * el.x;
    }
    float* dst = h + ((((size_t)b * U + u) * F + f) * T + t) * 2 * A;
    dst[a] = (float)hr;
    dst[A + a] = (float)hi;
  }
}

// y = the demodulated antenna grids yg [B][A][F][14] + the generator's grid noise (the draws of k_gen_rx);
// one thread per (b, f, t, a)
__global__ __launch_bounds__(256) void k_tc_y(nrx_gen_desc d, const double2* __restrict__ yg,
                                              const double* __restrict__ no_slot, float* __restrict__ y,
                                              float* __restrict__ y_re, float* __restrict__ y_im) {
  const int A = d.num_rx_ant, F = d.num_subcarriers, T = kT;
  const int64_t n = (int64_t)d.batch * F * T * A;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int a = (int)(i % A);
  const int64_t ft = i / A;                // (b, f, t)
  const int t = (int)(ft % T);
  const int f = (int)((ft / T) % F);
  const int64_t b = ft / ((int64_t)T * F);
  const double2 g = yg[(((size_t)b * A + a) * F + f) * T + t];
  const U4 r = draw(d, b, ST_NOISE, (uint32_t)((a * F + f) * T + t));
  const double2 z = box_muller(r.x, r.y);
  const double sd = sqrt((no_slot ? no_slot[b] : d.no) / 2.0);
  const float yr = (float)(g.x + sd * z.x), yi = (float)(g.y + sd * z.y);
  y[ft * 2 * A + a] = yr;
  y[ft * 2 * A + A + a] = yi;
  if (y_re) {
    y_re[ft * A + a] = yr;
    y_im[ft * A + a] = yi;
  }
}

struct TcWs {
  double2* xs;           // [B][U][Ls]  the transmitted samples
  double2* r;            // [B][A][Ls]  the noise-free received samples
  double2* g0;           // [B][U][A][L][NS]
  double* fd;            // [B][U][A][L][NS]
  double2* yg;           // [B][A][F][14]  the demodulated antenna grids
};

size_t tc_layout(const nrx_gen_desc& d, const nrx_gen_tc& tc, TcWs* w, void* base) {
  const size_t B = d.batch, U = d.num_tx, A = d.num_rx_ant, F = d.num_subcarriers;
  const size_t Ls = (size_t)slot_samples(tc.cp_length, tc.fft_size, kT);
  const size_t nsin = B * U * A * d.num_taps * d.num_sinusoids;
  Carver c(base);
  TcWs v;
  v.xs = c.take<double2>(B * U * Ls);
  v.r = c.take<double2>(B * A * Ls);
  v.g0 = c.take<double2>(nsin);
  v.fd = c.take<double>(nsin);
  v.yg = c.take<double2>(B * A * F * kT);
  if (w) *w = v;
  return c.bytes();
}

TcGen tc_gen(const nrx_gen_desc& d, const nrx_gen_chan& c, const nrx_gen_tc& tc) {
  TcGen g{};
  g.N = tc.fft_size, g.F = d.num_subcarriers;
  g.first_bin = tc.first_bin < 0 ? g.N / 2 - g.F / 2 : tc.first_bin;
  g.fs = (double)g.N * d.subcarrier_spacing;
  g.l_min = tc.l_min, g.l_max = tc_resolve_l_max(d, c, tc), g.ta = tc.timing_advance;
  int at = 0;
  for (int t = 0; t < kT; ++t) {
    g.wt[t] = at + tc.cp_length[t] - g.ta;
    at += tc.cp_length[t] + g.N;
  }
  g.Ls = at, g.n0 = tc.cp_length[0];
  return g;
}

}  // namespace

hipError_t launch_time_channel(const nrx_tc_io& io, hipStream_t st) {
  TcArgs p{};
  p.B = io.batch, p.U = io.num_tx, p.A = io.num_rx_ant, p.L = io.num_paths, p.NS = io.num_sinusoids;
  p.l_min = io.l_min, p.l_max = io.l_max, p.Ls = io.num_samples, p.n0 = io.n0, p.fs = io.sample_rate;
  p.tau = io.tau, p.fd = io.fd;
  p.g0 = reinterpret_cast<const double2*>(io.g0), p.x = reinterpret_cast<const double2*>(io.x);
  p.mix = io.rx_mix, p.r = reinterpret_cast<double2*>(io.r);
  return launch_tc_args(p, st);
}

int tc_resolve_l_max(const nrx_gen_desc& d, const nrx_gen_chan& c, const nrx_gen_tc& tc) {
  if (tc.l_max >= 0) return tc.l_max;
  double worst = 0.0;
  for (int u = 0; u < d.num_tx; ++u) worst = c.max_delay_s[u] > worst ? c.max_delay_s[u] : worst;
  const double v = ceil(worst * (double)tc.fft_size * d.subcarrier_spacing) + 6.0;
  return v < 1e6 ? (int)v : 1000000;       // beyond any span the check admits
}

size_t tc_workspace_bytes(const nrx_gen_desc& d, const nrx_gen_tc& tc) { return tc_layout(d, tc, nullptr, nullptr); }

hipError_t launch_tc_taps(const nrx_gen_desc& d, const nrx_gen_chan& c, const nrx_gen_tc& tc, const double* tau,
                          const double* spdp, double* gt, void* ws, hipStream_t st) {
  TcWs w;
  tc_layout(d, tc, &w, ws);
  const TcGen g = tc_gen(d, c, tc);
  const int64_t ngrp = (int64_t)d.batch * d.num_tx * d.num_rx_ant * d.num_taps, nsin = ngrp * d.num_sinusoids;
  k_tc_draws<<<(unsigned)((nsin + 255) / 256), 256, 0, st>>>(d, c, g, tau, spdp, w.g0, w.fd);
  k_tc_gbar<<<(unsigned)((ngrp * kT + 255) / 256), 256, 0, st>>>(g, d.num_sinusoids, ngrp * kT, w.g0, w.fd,
                                                                 reinterpret_cast<double2*>(gt));
  return hipGetLastError();
}

hipError_t launch_tc_rx(const nrx_gen_desc& d, const nrx_gen_chan& c, const nrx_gen_tc& tc, const double* x,
                        const double* tau, const double* gt, void* ws, const double* no_slot, float* y, float* h,
                        float* y_re, float* y_im, hipStream_t st) {
  TcWs w;
  tc_layout(d, tc, &w, ws);
  const TcGen g = tc_gen(d, c, tc);
  const int64_t B = d.batch, U = d.num_tx, A = d.num_rx_ant, F = d.num_subcarriers;
  if (hipError_t e = launch_ofdm(stage_ofdm(d, tc, (int)U, const_cast<double*>(x), w.xs), /*modulate=*/true, st)) return e;
  TcArgs p{};
  p.B = (int)B, p.U = (int)U, p.A = (int)A, p.L = d.num_taps, p.NS = d.num_sinusoids;
  p.l_min = g.l_min, p.l_max = g.l_max, p.Ls = g.Ls, p.n0 = g.n0, p.fs = g.fs;
  p.tau = tau, p.g0 = w.g0, p.fd = w.fd, p.x = w.xs, p.r = w.r;
  p.mix = c.rx_mix;
  if (hipError_t e = launch_tc_args(p, st)) return e;
  nrx_ofdm_io demod = stage_ofdm(d, tc, (int)A, w.yg, w.r);
  demod.timing_advance = tc.timing_advance;
  if (hipError_t e = launch_ofdm(demod, /*modulate=*/false, st)) return e;
  k_tc_y<<<(unsigned)((B * F * kT * A + 255) / 256), 256, 0, st>>>(d, w.yg, no_slot, y, y_re, y_im);
  if (h) {
    const int at = (int)(A * kT);
    int FB = 256 / at;
    if (FB > 4) FB = 4;
    k_tc_h<<<dim3((unsigned)((F + FB - 1) / FB), (unsigned)B), FB * at, 0, st>>>(
        d, g, FB, tau, reinterpret_cast<const double2*>(gt), h);
  }
  if (hipError_t e = hipGetLastError()) return e;
  const size_t row = (size_t)g.Ls * sizeof(double2);
  if (tc.r_out)
    if (hipError_t e = hipMemcpyAsync(tc.r_out, w.r, B * A * row, hipMemcpyDeviceToDevice, st)) return e;
  if (tc.x_out)
    if (hipError_t e = hipMemcpyAsync(tc.x_out, w.xs, B * U * row, hipMemcpyDeviceToDevice, st)) return e;
  return hipSuccess;
}

}  // namespace nrx
