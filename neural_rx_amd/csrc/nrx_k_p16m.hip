// nrx_k_p16m.hip -- the three-launch forward of the P16M strip tier (k_init / k_update /
// k_combine instantiations of nrx_device.inc), one code object of its own.
#include "nrx_device.inc"
#include "nrx_launch.inc"

namespace nrx {

hipError_t run_tier_p16m(const Args16& a, const Model16& W, const FwdPlan& pl, hipStream_t st, Prof* prof) {
  return Launch<P16M>::run(a, W, pl, st, prof);
}

hipError_t setup_tier_p16m() { return Launch<P16M>::setup(); }

}  // namespace nrx
