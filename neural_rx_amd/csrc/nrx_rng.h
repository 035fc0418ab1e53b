// nrx_rng.h -- the slot generator's counter-based random draws, shared by its kernels
// (nrx_synth.hip, nrx_cfo.hip): Philox4x32-10 with key = seed and counter = (element, slot lo,
// slot hi, stream), slot = slot_offset + b.  oracle/synth_ref.py states the same function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nrx.h"

namespace nrx {

// stream ids of the counter word c3 (oracle/synth_ref.py STREAM_*; ST_CFO: tests/cfo_ref.py;
// ST_DMRS: tests/dmrs_ref.py; ST_CIR: tests/cir_ref.py)
enum {
  ST_RE = 0, ST_ACTIVE = 1, ST_MCS = 2, ST_DELAY = 3, ST_TAP = 4, ST_NOISE = 5, ST_CFO = 6, ST_DMRS = 7, ST_CIR = 8
};

constexpr double kPi = 3.14159265358979323846;
constexpr double kCP = 1.07;      // symbol time = 1.07 / scs (normal cyclic prefix)

struct U4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                     uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
    const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
  }
  return {c0, c1, c2, c3};
}

__device__ __forceinline__ U4 draw(const nrx_gen_desc& d, int64_t b, int stream, uint32_t idx) {
  const uint64_t g = (uint64_t)(d.slot_offset + b);
  return philox(idx, (uint32_t)g, (uint32_t)(g >> 32), (uint32_t)stream, (uint32_t)d.seed,
                (uint32_t)(d.seed >> 32));
}

__device__ __forceinline__ double uni(uint32_t w) { return ((double)w + 0.5) * 0x1p-32; }

__device__ __forceinline__ double2 box_muller(uint32_t w0, uint32_t w1) {
  const double r = sqrt(-2.0 * log(uni(w0)));
  const double th = 2.0 * kPi * uni(w1);
  return make_double2(r * cos(th), r * sin(th));
}

}  // namespace nrx
