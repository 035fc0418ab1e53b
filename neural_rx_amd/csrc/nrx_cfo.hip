// nrx_cfo.hip -- per-user carrier frequency offset (CFO) in the slot generator, and the DMRS-based
// estimate and compensation of it on the receiver side (include/nrx.h "carrier frequency offset";
// tests/cfo_ref.py states the same functions in numpy f64).
//
//   k_cfo_apply     the impairment: per (slot, user) the transmit grid x [F][14] becomes
//                     x'[k][t] = e^{j theta_t} sum_m c[m - k] x[m][t],  c[d] = D_N(d + eps)
//                   a dense F x F complex Toeplitz product on v_mfma_f64_16x16x4_f64.  A workgroup owns
//                   one (slot, user) and kCfoTM output subcarriers, one 16-row tile per wave: M = output
//                   subcarriers, N = the 14 symbols padded to 16, K = input subcarriers.  The lags
//                   c[d] the workgroup needs are built once into LDS; the Toeplitz A operand of every
//                   K step is read from that table (lane (row i, k) takes c[m0 + k - i]), never
//                   from memory; x is staged through LDS in chunks of kCfoKC input subcarriers, split
//                   into a real and an imaginary plane (the B operands); four real MFMAs per complex
//                   step; the phasor e^{j theta_t} is applied to the accumulators.  No atomics: every
//                   output element has one owner and a fixed summation order.
//   k_cfo_h_phase   nrx_gen_cfo.h_with_phase: h *= e^{j theta_t} D_N(eps), the diagonal of the
//                   effective channel, in place on the f32 h of k_gen_rx
//   k_cfo_estimate  eps_hat from the own-pilot LS estimates of the closest DMRS symbol pairs;
//                   one workgroup per (slot, user), fixed-order f64 reduction
//   k_cfo_rotate    h_out = h_in e^{j sign 2 pi kCP eps_hat (t - t_ref)}
//
// The Dirichlet kernel.  D_N(v) = e^{j pi (N - 1) v / N} sin(pi v) / (N sin(pi v / N)).  With
// eps = n + r, n = rint(eps), and an integer lag d, sin(pi (d + eps)) = (-1)^(d + n) sin(pi r) and
// e^{j pi (d + eps)} = (-1)^(d + n) e^{j pi r}: the signs cancel and
//   c[d] = K (cot(phi) - j),  K = e^{j pi r} sin(pi r) / N,  phi = pi (q + r) / N,
// q = (d + n) mod N taken in (-N/2, N/2] (c is N-periodic), so that no argument of a sine grows
// with |d|.  r = 0 is the exact shift c[d] = [q == 0].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nrx.h"
#include "nrx_internal.h"
#include "nrx_rng.h"

namespace nrx {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kCfoTM = 64;        // output subcarriers of a workgroup: four waves, a 16-row tile each
constexpr int kCfoKC = 32;        // input subcarriers staged per K chunk
constexpr int kCfoThreads = 256;
constexpr int kPhaseChunk = 4096; // complex elements of one k_cfo_h_phase / k_cfo_rotate workgroup

struct DirK {
  double kr, ki;   // K
  double n, r;     // eps = n + r
  int N;
};

__device__ __forceinline__ DirK dir_k(double eps, int N) {
  DirK k;
  k.n = rint(eps);
  k.r = eps - k.n;
  k.N = N;
  double s, c;
  sincos(kPi * k.r, &s, &c);
  k.kr = c * s / N;
  k.ki = s * s / N;
  return k;
}

__device__ __forceinline__ double2 dir_lag(const DirK& k, int d) {
  double q = fmod((double)d + k.n, (double)k.N);      // exact
  if (2.0 * q > k.N) q -= k.N;
  if (2.0 * q <= -(double)k.N) q += k.N;
  if (k.r == 0.0) return make_double2(q == 0.0 ? 1.0 : 0.0, 0.0);
  double s, c;
  sincos(kPi * ((q + k.r) / k.N), &s, &c);
  const double cot = c / s;
  return make_double2(k.kr * cot + k.ki, k.ki * cot - k.kr);
}

// eps[b][u] in subcarrier spacings: the port's maximum, or a uniform draw in +-maximum
__device__ __forceinline__ double cfo_eps(const nrx_gen_desc& d, const GenCfo& c, int64_t b, int u) {
  if (c.constant) return c.eps_max[u];
  return c.eps_max[u] * (2.0 * uni(draw(d, b, ST_CFO, (uint32_t)u).x) - 1.0);
}

// e^{j theta_t}, theta_t = 2 pi eps (kCP t + (kCP - 1)): the rotation at the first sample after
// the cyclic prefix of symbol t
__device__ __forceinline__ double2 sym_phasor(double eps, int t) {
  double s, c;
  sincos(2.0 * kPi * (eps * (kCP * t + (kCP - 1.0))), &s, &c);
  return make_double2(c, s);
}

// grid (B * U, ceil(F / kCfoTM)); dynamic LDS: the lag table, then the two planes of the x chunk
__global__ __launch_bounds__(kCfoThreads) void k_cfo_apply(nrx_gen_desc d, GenCfo c, const double2* __restrict__ x,
                                                            const float* __restrict__ active,
                                                            double2* __restrict__ xp) {
  extern __shared__ double2 smem[];
  const int F = d.num_subcarriers, U = d.num_tx;
  const int64_t bu = blockIdx.x;
  const int64_t b = bu / U;
  const int u = (int)(bu % U);
  const int k0 = blockIdx.y * kCfoTM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double eps = cfo_eps(d, c, b, u);
  if (blockIdx.y == 0 && tid == 0 && c.eps_out) c.eps_out[bu] = eps;
  const double2* xb = x + (size_t)bu * F * kT;
  double2* ob = xp + (size_t)bu * F * kT;
  const int nrows = F - k0 < kCfoTM ? F - k0 : kCfoTM;
  if (eps == 0.0 || !(active[bu] > 0.0f)) {           // uniform: x' = x (zeros for an inactive port)
    for (int e = tid; e < nrows * kT; e += kCfoThreads) ob[(size_t)k0 * kT + e] = xb[(size_t)k0 * kT + e];
    return;
  }
  // lags d = m - k of every input subcarrier m < Fpad and output subcarrier k of this tile, at
  // index d + k0 + kCfoTM - 1
  const int Fpad = (F + kCfoKC - 1) / kCfoKC * kCfoKC;
  const int nl = Fpad + kCfoTM - 1;
  double2* tab = smem;
  double* xs_re = reinterpret_cast<double*>(smem + nl);
  double* xs_im = xs_re + kCfoKC * kTP;
  const DirK dk = dir_k(eps, c.fft_size);
  for (int i = tid; i < nl; i += kCfoThreads) tab[i] = dir_lag(dk, i - (k0 + kCfoTM - 1));

  const int col = lane & 15, kk = lane >> 4;
  const bool tile = k0 + 16 * wave < F;                // uniform over the wave
  // lane (row, kk) of the A operand at step s of the chunk at m0: c[(m0 + 4 s + kk) - (k0 + 16 wave + row)]
  const int abase = kCfoTM - 1 - 16 * wave - col + kk;
  f64x4 accr = {0.0, 0.0, 0.0, 0.0}, acci = {0.0, 0.0, 0.0, 0.0};
  for (int m0 = 0; m0 < F; m0 += kCfoKC) {
    __syncthreads();                                   // the table is there; the previous chunk has been read
    for (int e = tid; e < kCfoKC * kTP; e += kCfoThreads) {
      const int m = m0 + (e >> 4), t = e & 15;
      double2 v = make_double2(0.0, 0.0);
      if (m < F && t < kT) v = xb[(size_t)m * kT + t];
      xs_re[e] = v.x;
      xs_im[e] = v.y;
    }
    __syncthreads();
    if (tile) {
#pragma unroll
      for (int s = 0; s < kCfoKC / 4; ++s) {
        const double2 cv = tab[abase + m0 + 4 * s];
        const double xr = xs_re[(4 * s + kk) * kTP + col], xi = xs_im[(4 * s + kk) * kTP + col];
        accr = __builtin_amdgcn_mfma_f64_16x16x4f64(cv.x, xr, accr, 0, 0, 0);
        acci = __builtin_amdgcn_mfma_f64_16x16x4f64(cv.x, xi, acci, 0, 0, 0);
        accr = __builtin_amdgcn_mfma_f64_16x16x4f64(cv.y, -xi, accr, 0, 0, 0);
        acci = __builtin_amdgcn_mfma_f64_16x16x4f64(cv.y, xr, acci, 0, 0, 0);
      }
    }
  }
  // C / D layout of the f64 MFMA: column = lane & 15 (symbol), row = (lane >> 4) + 4 register
  if (tile && col < kT) {
    const double2 ph = sym_phasor(eps, col);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = k0 + 16 * wave + kk + 4 * r;
      if (k < F)
        ob[(size_t)k * kT + col] = make_double2(ph.x * accr[r] - ph.y * acci[r], ph.x * acci[r] + ph.y * accr[r]);
    }
  }
}

// h_out[e] = h_in[e] ph[t] over this workgroup's chunk of the [F][14][A] complex elements of one
// (slot, user) plane [F][14][2A] (re | im); f64 arithmetic, one f32 rounding.  In place is fine: a
// thread reads both halves of its element before it writes them.
__device__ __forceinline__ void rotate_chunk(const float* in, float* out, const double2* ph, int F, int A,
                                             int chunk) {
  const int n = F * kT * A;
  const int e1 = (chunk + 1) * kPhaseChunk < n ? (chunk + 1) * kPhaseChunk : n;
  for (int e = chunk * kPhaseChunk + threadIdx.x; e < e1; e += kCfoThreads) {
    const int a = e % A, ft = e / A;
    const double2 p = ph[ft % kT];
    const size_t i = (size_t)ft * 2 * A + a;
    const double hr = in[i], hi = in[i + A];
    out[i] = (float)(hr * p.x - hi * p.y);
    out[i + A] = (float)(hr * p.y + hi * p.x);
  }
}

// grid (B * U, ceil(F * 14 * A / kPhaseChunk))
__global__ __launch_bounds__(kCfoThreads) void k_cfo_h_phase(nrx_gen_desc d, GenCfo c, float* __restrict__ h) {
  __shared__ double2 ph[kTP];
  const int64_t bu = blockIdx.x;
  if (threadIdx.x < kT) {
    const double eps = cfo_eps(d, c, bu / d.num_tx, (int)(bu % d.num_tx));
    const double2 p = sym_phasor(eps, threadIdx.x), g = dir_lag(dir_k(eps, c.fft_size), 0);
    ph[threadIdx.x] = make_double2(p.x * g.x - p.y * g.y, p.x * g.y + p.y * g.x);
  }
  __syncthreads();
  float* hb = h + (size_t)bu * d.num_subcarriers * kT * 2 * d.num_rx_ant;
  rotate_chunk(hb, hb, ph, d.num_subcarriers, d.num_rx_ant, blockIdx.y);
}

// r = sum over the closest DMRS symbol pairs (D, D + g), antennas and own pilots of
// h_hat[p, D + g, a] conj(h_hat[p, D, a]); eps_hat = arg(r) / (2 pi kCP g).  One workgroup per
// (slot, user): every thread sums its items in index order, then a fixed tree in LDS.
__global__ __launch_bounds__(kCfoThreads) void k_cfo_estimate(nrx_cfo_io io) {
  __shared__ double red[2][kCfoThreads];
  const int U = io.num_tx, F = io.num_subcarriers, A = io.num_rx_ant, nd = io.num_dmrs_symbols;
  const int64_t bu = blockIdx.x;
  const int tid = threadIdx.x;
  int g = kT;
  for (int k = 0; k + 1 < nd; ++k) {
    const int gap = io.dmrs_symbols[k + 1] - io.dmrs_symbols[k];
    g = gap < g ? gap : g;
  }
  const int grp = io.cdm_group[bu % U];
  const int P = (F - grp + 1) >> 1;                    // own pilots: f = grp, grp + 2, ...
  if (nd < 2 || P < 1 || !(io.active[bu] > 0.0f)) {    // uniform
    if (tid == 0) io.eps[bu] = 0.0;
    return;
  }
  const float* hb = io.h_in + (size_t)bu * F * kT * 2 * A;
  double rr = 0.0, ri = 0.0;
  for (int k = 0; k + 1 < nd; ++k) {
    const int t0 = io.dmrs_symbols[k], t1 = io.dmrs_symbols[k + 1];
    if (t1 - t0 != g) continue;
    for (int e = tid; e < P * A; e += kCfoThreads) {
      const int a = e % A, p = e / A;
      const float* src = hb + (size_t)(grp + 2 * p) * kT * 2 * A + a;
      const double ar = src[t0 * 2 * A], ai = src[t0 * 2 * A + A];
      const double br = src[t1 * 2 * A], bi = src[t1 * 2 * A + A];
      rr += br * ar + bi * ai;
      ri += bi * ar - br * ai;
    }
  }
  red[0][tid] = rr;
  red[1][tid] = ri;
  __syncthreads();
  for (int o = kCfoThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    rr = red[0][0];
    ri = red[1][0];
    io.eps[bu] = rr == 0.0 && ri == 0.0 ? 0.0 : atan2(ri, rr) / (2.0 * kPi * kCP * g);
  }
}

// grid (B * U, ceil(F * 14 * A / kPhaseChunk))
__global__ __launch_bounds__(kCfoThreads) void k_cfo_rotate(nrx_cfo_io io) {
  __shared__ double2 ph[kTP];
  const int F = io.num_subcarriers, A = io.num_rx_ant;
  const int64_t bu = blockIdx.x;
  if (threadIdx.x < kT) {
    const int t = threadIdx.x;
    int tref = 0;
    if (io.ref_mode == NRX_CFO_REF_NEAREST_DMRS) {     // the generator's rule: the first listed nearest symbol
      int best = 1 << 30;
      for (int k = 0; k < io.num_dmrs_symbols; ++k) {
        const int dt = abs(t - io.dmrs_symbols[k]);
        if (dt < best) {
          best = dt;
          tref = io.dmrs_symbols[k];
        }
      }
    }
    double s, c;
    sincos(io.sign * (2.0 * kPi * kCP * io.eps[bu] * (double)(t - tref)), &s, &c);
    ph[t] = make_double2(c, s);
  }
  __syncthreads();
  const size_t off = (size_t)bu * F * kT * 2 * A;
  rotate_chunk(io.h_in + off, io.h_out + off, ph, F, A, blockIdx.y);
}

unsigned phase_chunks(int64_t F, int64_t A) { return (unsigned)((F * kT * A + kPhaseChunk - 1) / kPhaseChunk); }

}  // namespace

size_t cfo_workspace_bytes(const nrx_gen_desc& d) { return align256(gen_grid_elems(d) * sizeof(double2)); }

hipError_t launch_cfo_apply(const nrx_gen_desc& d, const GenCfo& c, const double* x, const float* active, double* xp,
                            hipStream_t st) {
  const int F = d.num_subcarriers;
  const int Fpad = (F + kCfoKC - 1) / kCfoKC * kCfoKC;
  const size_t lds = (size_t)(Fpad + kCfoTM - 1) * sizeof(double2) + 2 * kCfoKC * kTP * sizeof(double);
  const dim3 grid((unsigned)((int64_t)d.batch * d.num_tx), (unsigned)((F + kCfoTM - 1) / kCfoTM));
  k_cfo_apply<<<grid, kCfoThreads, lds, st>>>(d, c, reinterpret_cast<const double2*>(x), active,
                                               reinterpret_cast<double2*>(xp));
  return hipGetLastError();
}

hipError_t launch_cfo_h_phase(const nrx_gen_desc& d, const GenCfo& c, float* h, hipStream_t st) {
  const dim3 grid((unsigned)((int64_t)d.batch * d.num_tx), phase_chunks(d.num_subcarriers, d.num_rx_ant));
  k_cfo_h_phase<<<grid, kCfoThreads, 0, st>>>(d, c, h);
  return hipGetLastError();
}

hipError_t launch_cfo_estimate(const nrx_cfo_io& io, hipStream_t st) {
  k_cfo_estimate<<<(unsigned)((int64_t)io.batch * io.num_tx), kCfoThreads, 0, st>>>(io);
  return hipGetLastError();
}

hipError_t launch_cfo_rotate(const nrx_cfo_io& io, hipStream_t st) {
  const dim3 grid((unsigned)((int64_t)io.batch * io.num_tx), phase_chunks(io.num_subcarriers, io.num_rx_ant));
  k_cfo_rotate<<<grid, kCfoThreads, 0, st>>>(io);
  return hipGetLastError();
}

}  // namespace nrx
