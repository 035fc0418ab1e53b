// nrx_k_rr.hip -- the register-resident UpdateState launch (k_update_rr, nrx_rr.inc), one code
// object of its own; called by the f16 24-row tier's launch loop (Launch<P16>::run) for the
// update stages the plan gives it (plan_forward).
#include "nrx_device.inc"
#include "nrx_launch.inc"

namespace nrx {

#include "nrx_rr.inc"

hipError_t launch_update_rr(const BlockParams<P16>& bp, const StagePlan& sp, hipStream_t st) {
  const int items = sp.items, grid = sp.grid;
#ifdef NRX_STAMPS
  {
    // NRX_STAMP_RR = i: stamp the i-th RR launch of the process (0-based)
    static int launch_no = 0;
    static const int sel = getenv("NRX_STAMP_RR") ? atoi(getenv("NRX_STAMP_RR")) : -1;
    const int on = launch_no++ == sel;
    (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_nrx_stamp_on), &on, sizeof(int), 0, hipMemcpyHostToDevice, st);
  }
#endif
  if (sp.tail == TAIL_READOUT_WB) {
    if (sp.chp == 32) k_update_rr<32, TAIL_READOUT_WB><<<grid, 512, sp.lds, st>>>(bp, items);
    else k_update_rr<16, TAIL_READOUT_WB><<<grid, 512, sp.lds, st>>>(bp, items);
  } else {
    if (sp.chp == 32) k_update_rr<32, TAIL_AGG><<<grid, 512, sp.lds, st>>>(bp, items);
    else k_update_rr<16, TAIL_AGG><<<grid, 512, sp.lds, st>>>(bp, items);
  }
  return hipGetLastError();
}

hipError_t setup_update_rr() {
  hipError_t e = hipSuccess;
  auto set = [&](const void* f) {
    const hipError_t r = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kRrLds);
    if (r != hipSuccess) e = r;
  };
  set((const void*)k_update_rr<16, TAIL_AGG>);
  set((const void*)k_update_rr<32, TAIL_AGG>);
  set((const void*)k_update_rr<16, TAIL_READOUT_WB>);
  set((const void*)k_update_rr<32, TAIL_READOUT_WB>);
  return e;
}

}  // namespace nrx

#ifdef NRX_STAMPS
extern "C" int nrx_debug_rr_stamps(void* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(nrx::g_nrx_rr_stamps), (size_t)n * 64 * 8, 0, hipMemcpyDeviceToHost);
}
#endif
