// nrx_k_p16s.hip -- the three-launch forward of the P16S strip tier (k_init / k_update /
// k_combine instantiations of nrx_device.inc), one code object of its own.
#include "nrx_device.inc"
#include "nrx_launch.inc"

namespace nrx {

hipError_t run_tier_p16s(const Args16& a, const Model16& W, const FwdPlan& pl, hipStream_t st, Prof* prof) {
  return Launch<P16S>::run(a, W, pl, st, prof);
}

hipError_t setup_tier_p16s() { return Launch<P16S>::setup(); }

}  // namespace nrx
