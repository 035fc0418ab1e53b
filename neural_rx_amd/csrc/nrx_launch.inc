// nrx_launch.inc -- host-side launch templates shared by the kernel translation units
// (nrx_k_*.hip, nrx_dispatch.hip).  Each tier's kernels are instantiated and launched by ONE
// translation unit (its own code object), so a tier can be rebuilt alone.
#pragma once
namespace nrx {

// per-tier entry points (one translation unit each); every launcher executes the FwdPlan it is handed
// (plan_forward, nrx_dispatch.hip) and decides nothing
using Args16 = FwdArgs<_Float16, float, _Float16>;
using Model16 = ModelW<_Float16, float>;
hipError_t run_tier_p16(const Args16& a, const Model16& W, const FwdPlan& pl, hipStream_t st, Prof* prof);
hipError_t run_tier_p16m(const Args16& a, const Model16& W, const FwdPlan& pl, hipStream_t st, Prof* prof);
hipError_t run_tier_p16s(const Args16& a, const Model16& W, const FwdPlan& pl, hipStream_t st, Prof* prof);
hipError_t run_tier_p64(const FwdArgs<double, double, float>& a, const ModelW<double, double>& W, const FwdPlan& pl,
                        hipStream_t st, Prof* prof);
hipError_t setup_tier_p16(), setup_tier_p16m(), setup_tier_p16s(), setup_tier_p64();
// k_forward by MODE (0: bench-type, 1: general GZ, 2: staged z images); a2p = 8 / 16 / 32
hipError_t launch_kforward_m0(int a2p, const FusedParams<P16>& fp, int grid, hipStream_t st);
hipError_t launch_kforward_m1(int a2p, const FusedParams<P16>& fp, int grid, hipStream_t st);
hipError_t launch_kforward_m2(int a2p, const FusedParams<P16>& fp, int grid, hipStream_t st);
hipError_t setup_kforward_m0(), setup_kforward_m1(), setup_kforward_m2();
// the register-resident update stage (nrx_k_rr.hip, DESIGN.md section A.13)
hipError_t launch_update_rr(const BlockParams<P16>& bp, const StagePlan& sp, hipStream_t st);
hipError_t setup_update_rr();
// the whole-column launches (nrx_k_col.hip, DESIGN.md section 4)
hipError_t launch_init_col(const BlockParams<P16>& bp, const StagePlan& sp, hipStream_t st);
hipError_t launch_update_col(const BlockParams<P16>& bp, const StagePlan& sp, hipStream_t st);
hipError_t launch_fwd_col(const Args16& args, const Model16& W, const FwdPlan& pl, const FusedCtl& fc, hipStream_t st,
                          Prof* prof);
hipError_t setup_col();

// ---- the stage plan every forward launcher shares (Launch<P>::run, run_fused, launch_fwd_col)
// A forward is a list of stages: StateInit m = 0 .. num_init - 1 into s_out (m > 0 accumulating), then
// num_it updates on the ping-ponged state / aggregate planes.  The tail of a stage runs the NEXT
// iteration's aggregation MLP (the last StateInit: iteration 0's) or, in the last update, the readout.
// plan_stage fills what stage s's kernels read of it, in place: a, w, m, tail, agg and the heads.
// ro_tail (TAIL_READOUT or TAIL_READOUT_WB) is the caller's choice; the launch-wide fields strips, gz,
// inline_combine, norm_pre, pair and order_rev come from the FwdPlan.  What no kernel of the stage reads is
// zero: agg of the readout stage, m of an update.
template <class P>
static void plan_stage(BlockParams<P>& bp, const FwdArgs<typename P::WT, typename P::BT, typename P::S>& args,
                       const ModelW<typename P::WT, typename P::BT>& W, int num_it, int s, int ro_tail) {
  const int i = s - args.num_init;   // the update's iteration; < 0: StateInit s
  const bool last = i == num_it - 1;
  bp.a = args;
  if (i >= 0 && i % 2 == 0) {
    std::swap(bp.a.s_in, bp.a.s_out);
    std::swap(bp.a.a, bp.a.a_out);
  }
  for (int l = 0; l < 3; ++l) bp.w[l] = i < 0 ? W.init[s][l] : W.upd[i][l];
  bp.m = i < 0 ? s : 0;
  bp.tail = i < 0 ? (s == args.num_init - 1 ? TAIL_AGG : TAIL_NONE) : (last ? ro_tail : TAIL_AGG);
  for (int k = 0; k < 2; ++k)
    bp.agg[k] = last ? DenseW<typename P::WT, typename P::BT>{} : W.agg[i < 0 ? 0 : i + 1][k];
  for (int h = 0; h < args.H; ++h) {
    bp.llr[h][0] = W.llr[h][0];
    bp.llr[h][1] = W.llr[h][1];
  }
  bp.chest[0] = W.chest[0];
  bp.chest[1] = W.chest[1];
}

// The k_norm pre-pass: slots too long for the StateInit items to norm themselves (kNormFusedMaxQ) get
// their norm from a launch of its own, where the plan says so (FwdPlan::norm_pre = BlockParams::norm_pre).
template <class A>
static void norm_prepass(const A& args, const FwdPlan& pl, hipStream_t st, Prof* prof) {
  if (!pl.norm_pre) return;
  if (prof) prof->begin(K_NORM, st);
  k_norm<<<args.B, 1024, 0, st>>>(args.y, args.F * kT * 2 * args.A / 4, args.norm);
  if (prof) prof->end(K_NORM, st);
}

#ifdef NRX_STAMPS
// NRX_STAMP_LAUNCH = i stamps update i of the three-launch forward, -1 - m its StateInit m
static void stamp_select(int launch, hipStream_t st) {
  static const int sel = getenv("NRX_STAMP_LAUNCH") ? atoi(getenv("NRX_STAMP_LAUNCH")) : 0;
  const int on = launch == sel;
  (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_nrx_stamp_on), &on, sizeof(int), 0, hipMemcpyHostToDevice, st);
  (void)hipStreamSynchronize(st);
}
#else
static void stamp_select(int, hipStream_t) {}
#endif

template <class P>
struct Launch {
  using A = FwdArgs<typename P::WT, typename P::BT, typename P::S>;
  using MW = ModelW<typename P::WT, typename P::BT>;

  static hipError_t setup() {
    hipError_t e = hipSuccess;
    auto set = [&](const void* f, bool heads_wb = false) {
      hipError_t r = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, strip_lds_bytes<P>(heads_wb));
      if (r != hipSuccess) e = r;
    };
#define NRX_SET_INIT(A2P)                                     \
    set((const void*)k_init<P, A2P, TAIL_NONE>);              \
    set((const void*)k_init<P, A2P, TAIL_AGG>);
    NRX_SET_INIT(8) NRX_SET_INIT(16) NRX_SET_INIT(32)
#undef NRX_SET_INIT
    set((const void*)k_update<P, 16, TAIL_AGG>);
    set((const void*)k_update<P, 16, TAIL_READOUT>);
    set((const void*)k_update<P, 32, TAIL_AGG>);
    set((const void*)k_update<P, 32, TAIL_READOUT>);
    if constexpr (P::WLDS) {
      set((const void*)k_update<P, 16, TAIL_READOUT_WB>, true);
      set((const void*)k_update<P, 32, TAIL_READOUT_WB>, true);
    }
    return e;
  }

  template <int A2P>
  static void launch_init(dim3 grid, int L, hipStream_t st, const BlockParams<P>& bp, bool tail) {
    static_assert(init_cinp<A2P>(P::KC) <= kHID, "StateInit input wider than the strip image");
    if (tail) k_init<P, A2P, TAIL_AGG><<<grid, 512, L, st>>>(bp);
    else k_init<P, A2P, TAIL_NONE><<<grid, 512, L, st>>>(bp);
  }

  // one stage's launch: the launcher kind and the kernel variant the plan names
  static hipError_t launch_stage(const BlockParams<P>& bp, const StagePlan& sp, bool init, hipStream_t st) {
    const dim3 grid(sp.grid);
    const bool ch32 = sp.chp == 32;
    if constexpr (std::is_same<P, P16>::value) {   // the RR and column kernels exist for the 24-row tier only
      if (sp.kind == STAGE_COL) return init ? launch_init_col(bp, sp, st) : launch_update_col(bp, sp, st);
      if (sp.kind == STAGE_RR) return launch_update_rr(bp, sp, st);
    }
    if (init) {
      if (sp.chp == 8) launch_init<8>(grid, sp.lds, st, bp, sp.tail == TAIL_AGG);
      else if (sp.chp == 16) launch_init<16>(grid, sp.lds, st, bp, sp.tail == TAIL_AGG);
      else launch_init<32>(grid, sp.lds, st, bp, sp.tail == TAIL_AGG);
    } else if (sp.tail == TAIL_READOUT_WB) {   // paired readout items, the heads staged into WB
      if constexpr (P::WLDS) {
        if (ch32) k_update<P, 32, TAIL_READOUT_WB><<<grid, 512, sp.lds, st>>>(bp);
        else k_update<P, 16, TAIL_READOUT_WB><<<grid, 512, sp.lds, st>>>(bp);
      }
    } else if (sp.tail == TAIL_READOUT) {
      if (ch32) k_update<P, 32, TAIL_READOUT><<<grid, 512, sp.lds, st>>>(bp);
      else k_update<P, 16, TAIL_READOUT><<<grid, 512, sp.lds, st>>>(bp);
    } else {
      if (ch32) k_update<P, 32, TAIL_AGG><<<grid, 512, sp.lds, st>>>(bp);
      else k_update<P, 16, TAIL_AGG><<<grid, 512, sp.lds, st>>>(bp);
    }
    return hipSuccess;
  }

  static hipError_t run(const A& args, const MW& W, const FwdPlan& pl, hipStream_t st, Prof* prof) {
    auto B_ = [&](int k) { if (prof) prof->begin(k, st); };
    auto E_ = [&](int k) { if (prof) prof->end(k, st); };
    BlockParams<P> bp{};
    bp.inline_combine = pl.inline_combine;
    bp.gz = pl.gz;
    norm_prepass(args, pl, st, prof);
    bp.norm_pre = pl.norm_pre;
    // U > kInlineUsers: the leave-one-out combine runs as its own launch on the sp rows
    auto combine = [&](typename P::S* sp) {
      if (!pl.combine_launches()) return;
      dim3 g((args.F * kT * (kDS / P::EPC) + 255) / 256, args.B);
      B_(K_COMBINE);
      k_combine<P><<<g, 256, 0, st>>>(sp, args.active, args.U, args.F);
      E_(K_COMBINE);
    };
    // (bp.tail keeps TAIL_READOUT whichever readout variant runs the last stage)
    auto stage = [&](int s) {
      const StagePlan& sp = pl.st[s];
      plan_stage(bp, args, W, pl.num_it, s, TAIL_READOUT);
      bp.strips = sp.strips;
      bp.pair = sp.pair;
      bp.order_rev = sp.order_rev;
      return launch_stage(bp, sp, s < pl.num_init, st);
    };
    // StateInit, one launch per m (Var-IO), charged to the profiler as one stage
    B_(pl.st[0].kid);
    for (int m = 0; m < pl.num_init; ++m) {
      if (pl.st[m].kind == STAGE_STRIP) stamp_select(-1 - m, st);
      if (const hipError_t e = stage(m); e != hipSuccess) return e;
    }
    E_(pl.st[0].kid);
    combine(bp.a.a_out);
    for (int i = 0; i < pl.num_it; ++i) {
      const int s = pl.num_init + i;
      B_(pl.st[s].kid);
      stamp_select(i, st);
      if (const hipError_t e = stage(s); e != hipSuccess) return e;
      E_(pl.st[s].kid);
      if (i < pl.num_it - 1) combine(bp.a.a_out);
    }
    return hipGetLastError();
  }
};

// k_forward (PATH_KFWD0 .. 2): U <= 8 (with a workspace under 1 GB conv1 reads z from memory, GZ;
// otherwise the z image is staged in LDS), 1..M StateInit stages (Var-IO), up to three LLR heads, one of them in
// the paired-readout WB layout (TAIL_READOUT_WB) or all in the strip image (heads_x).  U = 3..8: a combine stage
// (k_combine's f32 pass, one item per (slot, strip)) before each update, whose conv1 then reads the a_u plane.
template <class P>
static hipError_t run_fused(const Args16& args, const Model16& W, const FwdPlan& pl, const FusedCtl& fc, hipStream_t st,
                            Prof* prof) {
  FusedParams<P> fp{};
  fp.sync = reinterpret_cast<FusedSync*>(fc.sync);
  fp.ninit = pl.num_init;
  fp.nst = pl.num_init + pl.num_it;
  fp.heads_x = pl.heads_x;
  fp.gz = pl.gz;
  fp.nls = 0;
  for (int s = 0; s < fp.ninit; ++s) {
    fp.kind[fp.nls] = 0;
    fp.pidx[fp.nls++] = s;
  }
  for (int i = 0; i < pl.num_it; ++i) {
    if (!pl.inline_combine) {
      fp.kind[fp.nls] = 2;
      fp.pidx[fp.nls++] = fp.ninit + i;
    }
    fp.kind[fp.nls] = 1;
    fp.pidx[fp.nls++] = fp.ninit + i;
  }
  fp.nq = pl.nq;
  fp.spin_limit = fc.spin_limit;
  fp.dbg_err = fc.dbg_err;
  norm_prepass(args, pl, st, prof);
  for (int s = 0; s < fp.nst; ++s) {
    BlockParams<P>& bp = fp.st[s];   // in place: FusedParams is several KB (pair, order_rev, gz stay 0)
    plan_stage(bp, args, W, pl.num_it, s, pl.heads_x ? TAIL_READOUT : TAIL_READOUT_WB);
    bp.inline_combine = pl.inline_combine;   // U > 2: the combine stages write a_u in place
    bp.norm_pre = pl.norm_pre;
    bp.strips = pl.st[s].strips;
  }
#ifdef NRX_STAMPS
  {
    const int on = getenv("NRX_STAMP_FUSED") ? 100 : 0;
    (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_nrx_stamp_on), &on, sizeof(int), 0, hipMemcpyHostToDevice, st);
    (void)hipStreamSynchronize(st);
  }
#endif
  if (prof) prof->begin(K_FUSED, st);
  hipError_t e = pl.path == PATH_KFWD0   ? launch_kforward_m0(pl.a2p, fp, pl.grid, st)
                 : pl.path == PATH_KFWD1 ? launch_kforward_m1(pl.a2p, fp, pl.grid, st)
                                         : launch_kforward_m2(pl.a2p, fp, pl.grid, st);
  if (e != hipSuccess) return e;
  if (prof) prof->end(K_FUSED, st);
  return hipGetLastError();
}

}  // namespace nrx
