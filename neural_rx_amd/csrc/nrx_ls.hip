// nrx_ls.hip -- the despreading least-squares channel estimator (include/nrx.h nrx_ls_estimate): from
// the received grid y and the known pilot table to h_hat [B][U][F][T][2A] (LS at the nearest own
// pilot) and the Aerial pilot list, for cover-coded DMRS ports (CDM group x frequency cover x time
// cover).  tests/dmrs_ref.py states the function in numpy float64; the slot generator
// (nrx_synth.hip, nrx_generate_slots_dmrs) gets its h_hat / h_ls outputs from the same launch.
//
//   k_ls_estimate   a workgroup owns (slot, tile of kLsTile subcarriers) for all U ports.  It stages
//                   the nd DMRS rows of y for its tile (plus kLsHalo subcarriers below it) and
//                   conj(p) / |p|^2 of the tile's slice of the pilot table into LDS once; then, a pass
//                   of up to ports_per_pass ports at a time,
//                     A  one thread per (DMRS symbol, comb position, port, antenna) despreads in f64
//                        and leaves the f32 estimate in LDS (and writes the Aerial list entry);
//                     B  the 14-symbol nearest-neighbour expansion of the pass: per port the tile's
//                        [f][t][2A] block is one contiguous range of h_hat, written as 16-byte stores
//                        (scalar stores where 2A is no multiple of 4 floats or h_hat is not 16-byte
//                        aligned).
//
// The halo: the nearest own pilot of the tile's first subcarrier is f - 1 for a port of CDM group 1,
// and under frequency despreading that pilot pairs with f - 3; the tile starts on a multiple of 4, so
// four subcarriers below it hold both and keep the pair (j, j ^ 1) of comb positions inside the staged
// range.  y is read once per tile (1 + kLsHalo / kLsTile times in all) instead of 14 U times; the
// kernel is bound by the h_hat write, 14 U / nd times the bytes it reads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nrx.h"
#include "nrx_internal.h"

namespace nrx {

namespace {

constexpr int kLsTile = 32;                     // subcarriers per workgroup, a multiple of 4
constexpr int kLsHalo = 4;
constexpr int kLsRows = kLsTile + kLsHalo;      // staged subcarriers
constexpr int kLsNJ = kLsRows / 2;              // staged comb positions per CDM group (even)
constexpr int kLsThreads = 256;
constexpr int kLsMaxH = 4 * kLsNJ * 4 * 32;     // f32 estimates kept in LDS per pass: 4 ports at nd = 4, A = 16

struct LsArgs {
  int B, U, F, A, nd;
  int despread_f, despread_t;
  int pmax;                 // (F + 1) / 2
  int ports_per_pass;
  int vec;                  // 16-byte stores
  int sym[4];
  unsigned knear;           // 2 bits per symbol t: position in sym[] of the first nearest DMRS symbol
  unsigned grp, focc, tocc; // bit u: cdm_group / focc / tocc of port u
  const float* y;
  const float* pilots;
  const float* active;
  float* h_hat;
  float* h_re;
  float* h_im;
};

// A2C: 2A at compile time (the index arithmetic of the write loop becomes multiply-shifts), 0 = any A
template <int A2C>
__global__ __launch_bounds__(kLsThreads) void k_ls_estimate(LsArgs p) {
  extern __shared__ __align__(16) unsigned char ls_smem[];
  const int A = p.A, A2 = A2C ? A2C : 2 * p.A, nd = p.nd, F = p.F, U = p.U;
  double2* sw = reinterpret_cast<double2*>(ls_smem);                        // [2][kLsNJ][4]
  float* sh = reinterpret_cast<float*>(sw + 2 * kLsNJ * 4);                 // [port][kLsNJ][nd][2A]
  float* sy = sh + p.ports_per_pass * kLsNJ * nd * A2;                      // [nd][kLsRows][2A]
  const int b = blockIdx.y;
  const int tile0 = blockIdx.x * kLsTile;
  const int sbase = tile0 - kLsHalo;            // first staged subcarrier (-4 for the first tile)
  const int jbase = sbase / 2;                  // ... and comb position; even, so j & 1 == jl & 1
  const int tn = F - tile0 < kLsTile ? F - tile0 : kLsTile;
  const int tid = threadIdx.x;

  for (int i = tid; i < nd * kLsRows * A2; i += kLsThreads) {
    const int c = i % A2, r = i / A2;
    const int lf = r % kLsRows, k = r / kLsRows;
    const int f = sbase + lf;
    sy[i] = f >= 0 && f < F ? p.y[(((size_t)b * F + f) * kT + p.sym[k]) * A2 + c] : 0.0f;
  }
  for (int i = tid; i < 2 * kLsNJ * nd; i += kLsThreads) {
    const int k = i % nd, jl = (i / nd) % kLsNJ, g = i / (nd * kLsNJ);
    const int j = jbase + jl;
    double2 w = make_double2(0.0, 0.0);
    if (j >= 0 && 2 * j + g < F) {
      const float* pp = p.pilots + (((size_t)g * p.pmax + j) * nd + k) * 2;
      const double pr = pp[0], pi = pp[1];
      const double den = pr * pr + pi * pi;
      w = make_double2(pr / den, -pi / den);
    }
    sw[(g * kLsNJ + jl) * 4 + k] = w;
  }
  __syncthreads();

  const int nj = p.despread_f ? 2 : 1, nk = p.despread_t ? 2 : 1;
  const int npl = nd * (F / 2);
  for (int u0 = 0; u0 < U; u0 += p.ports_per_pass) {
    const int pu = U - u0 < p.ports_per_pass ? U - u0 : p.ports_per_pass;
    // A: despread
    for (int i = tid; i < nd * kLsNJ * pu * A; i += kLsThreads) {
      const int a = i % A;
      int r = i / A;
      const int ul = r % pu;
      r /= pu;
      const int jl = r % kLsNJ, k = r / kLsNJ;
      const int u = u0 + ul;
      const int g = (p.grp >> u) & 1, wf = (p.focc >> u) & 1, wt = (p.tocc >> u) & 1;
      const int j = jbase + jl, f = 2 * j + g;
      const bool in_grid = j >= 0 && f < F;
      double hr = 0.0, hi = 0.0, ar = 0.0, ai = 0.0;
      if (in_grid && (!p.active || p.active[(size_t)b * U + u] > 0.0f)) {
        for (int dj = 0; dj < nj; ++dj) {
          const int j2 = jl ^ dj;
          double tr = 0.0, ti = 0.0;
          for (int dk = 0; dk < nk; ++dk) {
            const int k2 = k ^ dk;
            const double2 w = sw[(g * kLsNJ + j2) * 4 + k2];
            const float* yp = sy + (k2 * kLsRows + 2 * j2 + g) * A2;
            const double yr = yp[a], yi = yp[A + a];
            const double zr = yr * w.x - yi * w.y, zi = yr * w.y + yi * w.x;
            const bool neg = wt && (k2 & 1);
            tr += neg ? -zr : zr;
            ti += neg ? -zi : zi;
          }
          if (wf && (j2 & 1)) {
            tr = -tr;
            ti = -ti;
          }
          if (dj == 0) {
            ar = tr / nk;
            ai = ti / nk;
          }
          hr += tr;
          hi += ti;
        }
        hr /= nj * nk;
        hi /= nj * nk;
      }
      float* hp = sh + ((ul * kLsNJ + jl) * nd + k) * A2;
      hp[a] = (float)hr;
      hp[A + a] = (float)hi;
      // the Aerial list entry of a pilot of this tile (the halo's belong to the tile below)
      if (p.h_re && jl >= kLsHalo / 2 && in_grid) {
        const size_t o = ((((size_t)b * npl) + (size_t)k * (F / 2) + j) * U + u) * A + a;
        p.h_re[o] = (float)ar;
        p.h_im[o] = (float)ai;
      }
    }
    __syncthreads();
    // B: nearest-neighbour expansion, per port one contiguous range of tn * 14 * 2A floats
    if (p.h_hat) {
      for (int ul = 0; ul < pu; ++ul) {
        const int u = u0 + ul;
        const int g = (p.grp >> u) & 1;
        float* dst = p.h_hat + ((((size_t)b * U + u) * F + tile0) * kT) * A2;
        const float* hs = sh + ul * kLsNJ * nd * A2;
        if (p.vec) {
          const int nq = A2 / 4;
          for (int v = tid; v < tn * kT * nq; v += kLsThreads) {
            const int q = v % nq, r = v / nq;
            const int t = r % kT, f = tile0 + r / kT;
            const int fp = (f & 1) == g ? f : (f >= 1 ? f - 1 : f + 1);
            float4 val = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (fp < F) {
              const int k = (p.knear >> (2 * t)) & 3;
              val = *reinterpret_cast<const float4*>(hs + ((((fp - sbase) >> 1) * nd + k) * A2 + 4 * q));
            }
            reinterpret_cast<float4*>(dst)[v] = val;
          }
        } else {
          for (int e = tid; e < tn * kT * A2; e += kLsThreads) {
            const int c = e % A2, r = e / A2;
            const int t = r % kT, f = tile0 + r / kT;
            const int fp = (f & 1) == g ? f : (f >= 1 ? f - 1 : f + 1);
            float val = 0.0f;
            if (fp < F) {
              const int k = (p.knear >> (2 * t)) & 3;
              val = hs[(((fp - sbase) >> 1) * nd + k) * A2 + c];
            }
            dst[e] = val;
          }
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_ls_estimate(const nrx_ls_io& io, hipStream_t st) {
  LsArgs p{};
  p.B = io.batch, p.U = io.num_tx, p.F = io.num_subcarriers, p.A = io.num_rx_ant, p.nd = io.num_dmrs_symbols;
  p.despread_f = io.despread_f, p.despread_t = io.despread_t;
  p.pmax = (p.F + 1) / 2;
  const int A2 = 2 * p.A;
  const int per_port = kLsNJ * p.nd * A2;
  p.ports_per_pass = kLsMaxH / per_port < p.U ? kLsMaxH / per_port : p.U;
  p.vec = A2 % 4 == 0 && ((uintptr_t)io.h_hat & 15) == 0;
  for (int k = 0; k < p.nd; ++k) p.sym[k] = io.dmrs_symbols[k];
  for (int t = 0; t < kT; ++t) {
    int best = 0;
    for (int k = 1; k < p.nd; ++k)
      if (abs(t - p.sym[k]) < abs(t - p.sym[best])) best = k;
    p.knear |= (unsigned)best << (2 * t);
  }
  for (int u = 0; u < p.U; ++u) {
    p.grp |= (unsigned)io.cdm_group[u] << u;
    p.focc |= (unsigned)io.focc[u] << u;
    p.tocc |= (unsigned)io.tocc[u] << u;
  }
  p.y = io.y, p.pilots = io.pilots, p.active = io.active;
  p.h_hat = io.h_hat, p.h_re = io.h_ls_real, p.h_im = io.h_ls_imag;
  const size_t lds = 2 * kLsNJ * 4 * sizeof(double2) +
                     ((size_t)p.ports_per_pass * per_port + (size_t)p.nd * kLsRows * A2) * sizeof(float);
  const dim3 grid((unsigned)((p.F + kLsTile - 1) / kLsTile), (unsigned)p.B);
  switch (A2) {
    case 4: k_ls_estimate<4><<<grid, kLsThreads, lds, st>>>(p); break;
    case 8: k_ls_estimate<8><<<grid, kLsThreads, lds, st>>>(p); break;
    case 16: k_ls_estimate<16><<<grid, kLsThreads, lds, st>>>(p); break;
    case 32: k_ls_estimate<32><<<grid, kLsThreads, lds, st>>>(p); break;
    default: k_ls_estimate<0><<<grid, kLsThreads, lds, st>>>(p);
  }
  return hipGetLastError();
}

}  // namespace nrx
