// nrx_lmmse.hip -- classical baseline detector on the GPU: per-resource-element MIMO LMMSE
// equaliser + max-log QAM demapper (nrx_lmmse_detect, include/nrx.h), the detector of the
// reference's baselines (utils/baseline_rx.py:262-272: LinearDetector("lmmse", "bit", "maxlog")).
//
// Per RE (b, f, t), with s = no + err_var and H [A x U] the channel whose inactive columns are 0:
//   G = H^H H + s I,  x^ = G^-1 H^H y,  a_u = (G^-1)_uu,  mu_u = 1 - s a_u,
//   x~_u = x^_u / mu_u,  nu_u = s a_u / mu_u                (Sionna lmmse_equalizer, whitened)
//   llr_k = (min_{c: b_k = 0} |x~ - c|^2 - min_{c: b_k = 1} |x~ - c|^2) / nu_u
// The Gray QAM of TS 38.211 puts the even bits on the real axis and the odd bits on the imaginary
// axis, so every bit is a PAM search over the 2^(m/2) levels of its own axis.
//
// One lane per RE: lanes that are neighbours in (f, t) read neighbouring 2A-float rows of y and of
// every user's h plane, so a wave's loads are one contiguous run (dwordx4 per lane where A % 4 == 0
// and the rows are 16-byte aligned, scalar loads otherwise) and its LLR stores are contiguous per
// user.  H is never held whole: the antennas stream through four at a time (two for U >= 7, which
// keeps U = 8 at two waves per SIMD) while the lower
// triangle of G (real diagonal) and H^H y accumulate in registers; G = L D L^H is factorised in
// place, x^ comes from the two triangular solves and diag(G^-1) from the columns of L^-1.  The
// kernel is templated on U, so every index of the triangle is a compile-time constant and nothing
// is addressed at run time (no scratch).  f32 throughout, no atomics: outputs are deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nrx.h"
#include "nrx_internal.h"

namespace nrx {

namespace {

constexpr int kLmmseBlock = 256;
constexpr float kMuMin = 1e-6f;     // below this the unbiasing 1 / mu is meaningless: LLRs are 0

struct LmmseArgs {
  int64_t n;          // B * F * T
  int FT, A, BS, dmrs_mask, num_mcs;
  int vst;            // llr is 16-byte aligned: bits_stride 4 / 6 rows take dwordx4 / dwordx2 stores
  int mcs_bits[8];
  float s;
  const float* y;
  const float* h;
  const float* active;
  const uint8_t* mcs;
  float* llr;
};

// level j of the 2^NB-PAM of one axis; bit q of j is the axis' q-th bit (TS 38.211 5.1.3-5.1.5
// without the 1 / sqrt(2), 1 / sqrt(10), 1 / sqrt(42) scale)
template <int NB>
__host__ __device__ __forceinline__ constexpr float pam_level(int j) {
  const float s0 = 1.0f - 2.0f * (float)(j & 1);
  const float s1 = 1.0f - 2.0f * (float)((j >> 1) & 1);
  const float s2 = 1.0f - 2.0f * (float)((j >> 2) & 1);
  return NB == 1 ? s0 : (NB == 2 ? s0 * (2.0f - s1) : s0 * (4.0f - s1 * (2.0f - s2)));
}

// max-log LLRs of the NB bits of one axis: out[q] = (min_{b_q = 0} - min_{b_q = 1}) (x - level)^2 / nu
template <int NB>
__host__ __device__ __forceinline__ void pam_llr(float x, float inv_nu, float scale, float (&out)[3]) {
  float d0[NB], d1[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) d0[q] = d1[q] = 3.0e38f;
#pragma unroll
  for (int j = 0; j < (1 << NB); ++j) {
    const float e = x - pam_level<NB>(j) * scale;
    const float d = e * e;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      if ((j >> q) & 1) d1[q] = fminf(d1[q], d);
      else d0[q] = fminf(d0[q], d);
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) out[q] = 0.0f;
#pragma unroll
  for (int q = 0; q < NB; ++q) out[q] = (d0[q] - d1[q]) * inv_nu;
}

// RE i = (b * F + f) * T + t of the batch: all of its users.  Host-callable too, so that the
// arithmetic can be run and checked (and put under a host sanitizer) without a device.
template <int U, bool VEC>
__host__ __device__ __forceinline__ void lmmse_re(const LmmseArgs& p, int64_t i) {
  const int64_t b = i / p.FT;
  const int ft = (int)(i - b * p.FT);
  const int t = ft % kT;
  const int A = p.A;
  const bool data = !((p.dmrs_mask >> t) & 1);

  bool act[U];
#pragma unroll
  for (int u = 0; u < U; ++u) act[u] = p.active[b * U + u] > 0.0f;

  float xr[U], xi[U], mu[U], inv_nu[U];
#pragma unroll
  for (int u = 0; u < U; ++u) xr[u] = xi[u] = mu[u] = inv_nu[u] = 0.0f;

  if (data) {
    // lower triangle of G = H^H H + s I (gr[i][i] real) and z = H^H y
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
    if (VEC && U >= 7) {
      // two antennas per step (dwordx2): sixteen float4 in flight on top of the 64-float triangle
      // would leave U = 8 one wave per SIMD
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
#define NRX_LMMSE_ANT(C)                                  \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {         \
    hr[u] = act[u] ? h2r[u].C : 0.0f;                     \
    hi[u] = act[u] ? h2i[u].C : 0.0f;                     \
  }                                                       \
  accumulate(hr, hi, y2r.C, y2i.C);
        NRX_LMMSE_ANT(x)
        NRX_LMMSE_ANT(y)
#undef NRX_LMMSE_ANT
      }
    } else if (VEC) {
      for (int a0 = 0; a0 < A; a0 += 4) {
        const float4 y4r = *reinterpret_cast<const float4*>(yrow + a0);
        const float4 y4i = *reinterpret_cast<const float4*>(yrow + A + a0);
        float4 h4r[U], h4i[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          h4r[u] = *reinterpret_cast<const float4*>(hrow + u * hplane + a0);
          h4i[u] = *reinterpret_cast<const float4*>(hrow + u * hplane + A + a0);
        }
        float hr[U], hi[U];
#define NRX_LMMSE_ANT(C)                                  \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {         \
    hr[u] = act[u] ? h4r[u].C : 0.0f;                     \
    hi[u] = act[u] ? h4i[u].C : 0.0f;                     \
  }                                                       \
  accumulate(hr, hi, y4r.C, y4i.C);
        NRX_LMMSE_ANT(x)
        NRX_LMMSE_ANT(y)
        NRX_LMMSE_ANT(z)
        NRX_LMMSE_ANT(w)
#undef NRX_LMMSE_ANT
      }
    } else {
      for (int a = 0; a < A; ++a) {
        float hr[U], hi[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float vr = hrow[u * hplane + a], vi = hrow[u * hplane + A + a];
          hr[u] = act[u] ? vr : 0.0f;
          hi[u] = act[u] ? vi : 0.0f;
        }
        accumulate(hr, hi, yrow[a], yrow[A + a]);
      }
    }
#pragma unroll
    for (int r = 0; r < U; ++r) gr[r][r] += p.s;

    // G = L D L^H in place: unit lower L in gr/gi[r][c] (c < r), D in gr[c][c], 1 / D in dinv
    float dinv[U];
#pragma unroll
    for (int c = 0; c < U; ++c) {
      float d = gr[c][c];
#pragma unroll
      for (int k = 0; k < c; ++k) d -= (gr[c][k] * gr[c][k] + gi[c][k] * gi[c][k]) * gr[k][k];
      gr[c][c] = d;
      dinv[c] = 1.0f / d;
#pragma unroll
      for (int r = c + 1; r < U; ++r) {
        float ar = gr[r][c], ai = gi[r][c];
#pragma unroll
        for (int k = 0; k < c; ++k) {
          // L_rk d_k conj(L_ck)
          const float vr = gr[r][k] * gr[k][k], vi = gi[r][k] * gr[k][k];
          ar -= vr * gr[c][k] + vi * gi[c][k];
          ai -= vi * gr[c][k] - vr * gi[c][k];
        }
        gr[r][c] = ar * dinv[c];
        gi[r][c] = ai * dinv[c];
      }
    }
    // w = L^-1 z, v = D^-1 w, x^ = L^-H v
#pragma unroll
    for (int r = 0; r < U; ++r) {
#pragma unroll
      for (int k = 0; k < r; ++k) {
        zr[r] -= gr[r][k] * zr[k] - gi[r][k] * zi[k];
        zi[r] -= gr[r][k] * zi[k] + gi[r][k] * zr[k];
      }
    }
#pragma unroll
    for (int r = U - 1; r >= 0; --r) {
      float ar = zr[r] * dinv[r], ai = zi[r] * dinv[r];
#pragma unroll
      for (int k = r + 1; k < U; ++k) {
        // conj(L_kr) x^_k
        ar -= gr[k][r] * xr[k] + gi[k][r] * xi[k];
        ai -= gr[k][r] * xi[k] - gi[k][r] * xr[k];
      }
      xr[r] = ar;
      xi[r] = ai;
    }
    // a_u = (G^-1)_uu = sum_{k >= u} |(L^-1)_ku|^2 / d_k, column u of L^-1 by forward substitution
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float mr[U], mi[U];
      float a = dinv[u];
#pragma unroll
      for (int r = u + 1; r < U; ++r) {
        float ar = -gr[r][u], ai = -gi[r][u];
#pragma unroll
        for (int k = u + 1; k < r; ++k) {
          ar -= gr[r][k] * mr[k] - gi[r][k] * mi[k];
          ai -= gr[r][k] * mi[k] + gi[r][k] * mr[k];
        }
        mr[r] = ar;
        mi[r] = ai;
        a += (ar * ar + ai * ai) * dinv[r];
      }
      const float sa = p.s * a;
      mu[u] = 1.0f - sa;
      inv_nu[u] = mu[u] / sa;
    }
  }

#pragma unroll
  for (int u = 0; u < U; ++u) {
    float o[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (data && act[u] && mu[u] >= kMuMin) {
      int mi_ = p.mcs ? (int)p.mcs[b * U + u] : 0;
      mi_ = mi_ < p.num_mcs ? mi_ : p.num_mcs - 1;
      const int m = p.mcs_bits[mi_];
      const float rmu = 1.0f / mu[u];
      const float er = xr[u] * rmu, ei = xi[u] * rmu;
      float lr[3], li[3];
      if (m == 2) {
        pam_llr<1>(er, inv_nu[u], 0.70710678118654752f, lr);
        pam_llr<1>(ei, inv_nu[u], 0.70710678118654752f, li);
      } else if (m == 4) {
        pam_llr<2>(er, inv_nu[u], 0.31622776601683794f, lr);
        pam_llr<2>(ei, inv_nu[u], 0.31622776601683794f, li);
      } else {
        pam_llr<3>(er, inv_nu[u], 0.15430334996209191f, lr);
        pam_llr<3>(ei, inv_nu[u], 0.15430334996209191f, li);
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        o[2 * q] = lr[q];
        o[2 * q + 1] = li[q];
      }
    }
    const int BS = p.BS;
    float* dst = p.llr + (((size_t)b * U + u) * p.FT + ft) * BS;
    if (p.vst && BS == 4) {
      *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    } else if (p.vst && BS == 6) {
      *reinterpret_cast<float2*>(dst) = make_float2(o[0], o[1]);
      *reinterpret_cast<float2*>(dst + 2) = make_float2(o[2], o[3]);
      *reinterpret_cast<float2*>(dst + 4) = make_float2(o[4], o[5]);
    } else {
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (k < BS) dst[k] = o[k];
      for (int k = 6; k < BS; ++k) dst[k] = 0.0f;
    }
  }
}

template <int U, bool VEC>
__global__ __launch_bounds__(kLmmseBlock) void k_lmmse(LmmseArgs p) {
  const int64_t i = (int64_t)blockIdx.x * kLmmseBlock + threadIdx.x;
  if (i < p.n) lmmse_re<U, VEC>(p, i);
}

template <int U>
void launch_u(const LmmseArgs& a, bool vec, hipStream_t st) {
  const unsigned grid = (unsigned)((a.n + kLmmseBlock - 1) / kLmmseBlock);
  if (vec) k_lmmse<U, true><<<grid, kLmmseBlock, 0, st>>>(a);
  else k_lmmse<U, false><<<grid, kLmmseBlock, 0, st>>>(a);
}

}  // namespace

hipError_t launch_lmmse(const nrx_lmmse_io& io, hipStream_t st) {
  LmmseArgs a;
  a.FT = io.num_subcarriers * io.num_symbols;
  a.n = (int64_t)io.batch * a.FT;
  a.A = io.num_rx_ant;
  a.BS = io.bits_stride;
  a.dmrs_mask = io.dmrs_symbol_mask;
  a.num_mcs = io.num_mcs;
  for (int m = 0; m < 8; ++m) a.mcs_bits[m] = m < io.num_mcs ? io.mcs_bits[m] : io.mcs_bits[0];
  a.s = (float)(io.no + io.err_var);
  a.y = io.y;
  a.h = io.h;
  a.active = io.active;
  a.mcs = io.mcs;
  a.llr = io.llr;
  // dwordx4 loads need A % 4 == 0 and 16-byte aligned bases (rows are 8A bytes); else scalar loads
  const bool vec = io.num_rx_ant % 4 == 0 && (((uintptr_t)io.y | (uintptr_t)io.h) & 15) == 0;
  a.vst = ((uintptr_t)io.llr & 15) == 0;
  switch (io.num_tx) {
    case 1: launch_u<1>(a, vec, st); break;
    case 2: launch_u<2>(a, vec, st); break;
    case 3: launch_u<3>(a, vec, st); break;
    case 4: launch_u<4>(a, vec, st); break;
    case 5: launch_u<5>(a, vec, st); break;
    case 6: launch_u<6>(a, vec, st); break;
    case 7: launch_u<7>(a, vec, st); break;
    case 8: launch_u<8>(a, vec, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace nrx
