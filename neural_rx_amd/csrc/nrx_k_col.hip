// nrx_k_col.hip -- the whole-column register-resident launches (k_init_col, k_update_col;
// nrx_col.inc), one code object of their own; called by the f16 24-row tier's launch loop
// (Launch<P16>::run) for the stages the plan gives them (plan_forward); the stage parameters of the
// one-launch column forward are nrx_launch.inc's plan_stage, as for every launcher.
#include "nrx_device.inc"
#include "nrx_launch.inc"

namespace nrx {

#include "nrx_rr.inc"
#include "nrx_col.inc"

#ifdef NRX_STAMPS
static void col_stamp_select(hipStream_t st) {
  // NRX_STAMP_COL = i: stamp the i-th column launch of the process (0-based)
  static int launch_no = 0;
  static const int sel = getenv("NRX_STAMP_COL") ? atoi(getenv("NRX_STAMP_COL")) : -1;
  const int on = launch_no++ == sel;
  (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_nrx_stamp_on), &on, sizeof(int), 0, hipMemcpyHostToDevice, st);
}
#else
static void col_stamp_select(hipStream_t) {}
#endif

hipError_t launch_init_col(const BlockParams<P16>& bp, const StagePlan& sp, hipStream_t st) {
  const int items = sp.items, grid = sp.grid;
  col_stamp_select(st);
  // the last StateInit launch runs iteration 0's aggregation MLP (TAIL_AGG), earlier ones (Var-IO) none
  const bool agg = sp.tail == TAIL_AGG;
  // the plan's variant (lean: one item per workgroup, TAIL_AGG; plan_forward)
  if (sp.variant != COL_GENERIC) {
    if (!sp.one || !agg) return hipErrorInvalidValue;
    k_init_col<TAIL_AGG, ColLean<true>><<<grid, 512, sp.lds, st>>>(bp, items);
  } else if (sp.one) {
    if (agg) k_init_col<TAIL_AGG><<<grid, 512, sp.lds, st>>>(bp, items);
    else k_init_col<TAIL_NONE><<<grid, 512, sp.lds, st>>>(bp, items);
  } else {
    if (agg) k_init_col_multi<TAIL_AGG><<<grid, 512, sp.lds, st>>>(bp, items);
    else k_init_col_multi<TAIL_NONE><<<grid, 512, sp.lds, st>>>(bp, items);
  }
  return hipGetLastError();
}

hipError_t launch_update_col(const BlockParams<P16>& bp, const StagePlan& sp, hipStream_t st) {
  const int items = sp.items, grid = sp.grid, L = sp.lds;
  const bool ch32 = sp.chp == 32, one = sp.one;   // one item per workgroup, or the looping kernel
  col_stamp_select(st);
  if (sp.variant != COL_GENERIC) {   // lean: one item per workgroup, CHP = 16 (plan_forward)
    if (!one || ch32) return hipErrorInvalidValue;
    if (sp.tail != TAIL_READOUT_WB) k_update_col<16, TAIL_AGG, ColLean<true>><<<grid, 512, L, st>>>(bp, items);
    else if (sp.variant == COL_LEAN) k_update_col<16, TAIL_READOUT_WB, ColLean<true>><<<grid, 512, L, st>>>(bp, items);
    else k_update_col<16, TAIL_READOUT_WB, ColLean<false>><<<grid, 512, L, st>>>(bp, items);
  } else if (sp.tail == TAIL_READOUT_WB) {
    if (ch32) {
      if (one) k_update_col<32, TAIL_READOUT_WB><<<grid, 512, L, st>>>(bp, items);
      else k_update_col_multi<32, TAIL_READOUT_WB><<<grid, 512, L, st>>>(bp, items);
    } else {
      if (one) k_update_col<16, TAIL_READOUT_WB><<<grid, 512, L, st>>>(bp, items);
      else k_update_col_multi<16, TAIL_READOUT_WB><<<grid, 512, L, st>>>(bp, items);
    }
  } else {
    if (ch32) {
      if (one) k_update_col<32, TAIL_AGG><<<grid, 512, L, st>>>(bp, items);
      else k_update_col_multi<32, TAIL_AGG><<<grid, 512, L, st>>>(bp, items);
    } else {
      if (one) k_update_col<16, TAIL_AGG><<<grid, 512, L, st>>>(bp, items);
      else k_update_col_multi<16, TAIL_AGG><<<grid, 512, L, st>>>(bp, items);
    }
  }
  return hipGetLastError();
}

// the one-launch column forward (k_fwd_col): every item stages its weights, so the plan takes it for at most one
// item per CU and stage (plan_forward)
hipError_t launch_fwd_col(const Args16& args, const Model16& W, const FwdPlan& pl, const FusedCtl& fc, hipStream_t st,
                          Prof* prof) {
  ColFwdParams fp{};
  fp.sync = reinterpret_cast<FusedSync*>(fc.sync);
  fp.nst = pl.num_init + pl.num_it;
  fp.nq = pl.nq;
  fp.spin_limit = fc.spin_limit;
  fp.dbg_err = fc.dbg_err;
  norm_prepass(args, pl, st, prof);
  for (int s = 0; s < fp.nst; ++s) {
    BlockParams<P16>& bp = fp.st[s];   // in place (pair, order_rev stay 0)
    plan_stage(bp, args, W, pl.num_it, s, TAIL_READOUT_WB);
    bp.inline_combine = pl.inline_combine;
    bp.norm_pre = pl.norm_pre;
    bp.strips = pl.st[s].strips;
    bp.gz = pl.gz;
  }
  col_stamp_select(st);
  if (prof) prof->begin(K_FWD_COL, st);
  k_fwd_col<16><<<pl.grid, 512, pl.lds, st>>>(fp);
  if (prof) prof->end(K_FWD_COL, st);
  return hipGetLastError();
}

hipError_t setup_col() {
  hipError_t e = hipSuccess;
  auto set = [&](const void* f) {
    const hipError_t r = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kColLds);
    if (r != hipSuccess) e = r;
  };
  set((const void*)k_init_col<TAIL_AGG>);
  set((const void*)k_init_col<TAIL_NONE>);
  set((const void*)k_init_col_multi<TAIL_AGG>);
  set((const void*)k_init_col_multi<TAIL_NONE>);
  set((const void*)k_update_col<16, TAIL_AGG>);
  set((const void*)k_update_col<32, TAIL_AGG>);
  set((const void*)k_update_col<16, TAIL_READOUT_WB>);
  set((const void*)k_update_col<32, TAIL_READOUT_WB>);
  set((const void*)k_update_col_multi<16, TAIL_AGG>);
  set((const void*)k_update_col_multi<32, TAIL_AGG>);
  set((const void*)k_update_col_multi<16, TAIL_READOUT_WB>);
  set((const void*)k_update_col_multi<32, TAIL_READOUT_WB>);
  set((const void*)k_fwd_col<16>);
  set((const void*)k_init_col<TAIL_AGG, ColLean<true>>);
  set((const void*)k_update_col<16, TAIL_AGG, ColLean<true>>);
  set((const void*)k_update_col<16, TAIL_READOUT_WB, ColLean<true>>);
  set((const void*)k_update_col<16, TAIL_READOUT_WB, ColLean<false>>);
  return e;
}

}  // namespace nrx

#ifdef NRX_STAMPS
extern "C" int nrx_debug_col_stamps(void* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(nrx::g_nrx_rr_stamps), (size_t)n * 64 * 8, 0, hipMemcpyDeviceToHost);
}
#endif
