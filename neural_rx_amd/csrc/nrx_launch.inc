// nrx_launch.inc -- host-side launch templates shared by the kernel translation units
// (nrx_k_*.hip, nrx_dispatch.hip).  Each tier's kernels are instantiated and launched by ONE
// translation unit (its own code object), so a tier can be rebuilt alone.
#pragma once
namespace nrx {

// per-tier entry points (one translation unit each)
hipError_t run_tier_p16(const FwdArgs<_Float16, float, _Float16>& a, const ModelW<_Float16, float>& W, int num_it,
                        hipStream_t st, Prof* prof, int update_rr);
hipError_t run_tier_p16m(const FwdArgs<_Float16, float, _Float16>& a, const ModelW<_Float16, float>& W, int num_it,
                         hipStream_t st, Prof* prof);
hipError_t run_tier_p16s(const FwdArgs<_Float16, float, _Float16>& a, const ModelW<_Float16, float>& W, int num_it,
                         hipStream_t st, Prof* prof);
hipError_t run_tier_p64(const FwdArgs<double, double, float>& a, const ModelW<double, double>& W, int num_it,
                        hipStream_t st, Prof* prof);
hipError_t setup_tier_p16();
hipError_t setup_tier_p16m();
hipError_t setup_tier_p16s();
hipError_t setup_tier_p64();
// k_forward by MODE (0: bench-type, 1: general GZ, 2: staged z images); a2p = 8 / 16 / 32
hipError_t launch_kforward_m0(int a2p, const FusedParams<P16>& fp, int grid, hipStream_t st);
hipError_t launch_kforward_m1(int a2p, const FusedParams<P16>& fp, int grid, hipStream_t st);
hipError_t launch_kforward_m2(int a2p, const FusedParams<P16>& fp, int grid, hipStream_t st);
// the register-resident update stage (nrx_k_rr.hip, DESIGN.md section A.13)
bool update_rr_applicable(const FwdArgs<_Float16, float, _Float16>& a, bool gz, bool inline_combine, bool last);
hipError_t launch_update_rr(const BlockParams<P16>& bp, bool last, hipStream_t st);
hipError_t setup_update_rr();
// the whole-column launches (nrx_k_col.hip, DESIGN.md section 4)
bool col_init_applicable(const FwdArgs<_Float16, float, _Float16>& a);
bool update_col_applicable(const FwdArgs<_Float16, float, _Float16>& a, bool gz, bool last, int sched);
hipError_t launch_init_col(const BlockParams<P16>& bp, hipStream_t st);
hipError_t launch_update_col(const BlockParams<P16>& bp, bool last, hipStream_t st);
hipError_t setup_col();
bool fwd_col_applicable(const FwdArgs<_Float16, float, _Float16>& a, int num_it, const FusedCtl& fc);
hipError_t launch_fwd_col(const FwdArgs<_Float16, float, _Float16>& args, const ModelW<_Float16, float>& W, int num_it,
                          hipStream_t st, Prof* prof, const FusedCtl& fc);
hipError_t setup_kforward_m0();
hipError_t setup_kforward_m1();
hipError_t setup_kforward_m2();


// CUs of the current device for the pairing / strip-tier heuristics, queried once per
// device on first use (ADVICE r02: a single cached value was wrong for other devices)
constexpr int kMaxDevices = 64;
static int g_cu_count[kMaxDevices];
static int cu_count() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256;
  if (g_cu_count[dev] <= 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 256;
    g_cu_count[dev] = cus;
  }
  return g_cu_count[dev];
}

// ---- the stage plan every forward launcher shares (Launch<P>::run, run_fused, launch_fwd_col)
// A forward is a list of stages: StateInit m = 0 .. num_init - 1 into s_out (m > 0 accumulating), then
// num_it updates on the ping-ponged state / aggregate planes.  The tail of a stage runs the NEXT
// iteration's aggregation MLP (the last StateInit: iteration 0's) or, in the last update, the readout.
// plan_stage fills what stage s's kernels read of it, in place: a, w, m, tail, agg and the heads.
// ro_tail (TAIL_READOUT or TAIL_READOUT_WB) is the caller's choice, and so are the launch-wide fields
// strips, gz, inline_combine, norm_pre, pair and order_rev.  What no kernel of the stage reads is
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
// their norm from a launch of its own.  Returns BlockParams::norm_pre.
template <class A>
static bool norm_prepass(const A& args, hipStream_t st, Prof* prof) {
  const int nq = args.F * kT * 2 * args.A / 4;
  if (nq <= kNormFusedMaxQ) return false;
  if (prof) prof->begin(K_NORM, st);
  k_norm<<<args.B, 1024, 0, st>>>(args.y, nq, args.norm);
  if (prof) prof->end(K_NORM, st);
  return true;
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

  static hipError_t run(const A& args, const MW& W, int num_it, hipStream_t st, Prof* prof, int update_rr = 0) {
    const int strips = (args.F + P::FO - 1) / P::FO;
    constexpr int L = strip_lds_bytes<P>();
    const bool ch32 = 2 * args.A > 16;
    auto B_ = [&](int k) { if (prof) prof->begin(k, st); };
    auto E_ = [&](int k) { if (prof) prof->end(k, st); };
    BlockParams<P> bp{};
    bp.inline_combine = args.U <= kInlineUsers;
    if constexpr (std::is_same<P, P16>::value)   // 24-row strips, the workspace within GZ's offsets
      bp.gz = NRX_UPDATE_GZ != 0 && args.ws_bytes < kGzOob && args.pe16 != nullptr;
    bp.strips = strips;
    bp.norm_pre = norm_prepass(args, st, prof);
    int launch_no = 0;
    // U > kInlineUsers: the leave-one-out combine runs as its own launch on the sp rows
    auto combine = [&](typename P::S* sp) {
      if (bp.inline_combine) return;
      dim3 g((args.F * kT * (kDS / P::EPC) + 255) / 256, args.B);
      B_(K_COMBINE);
      k_combine<P><<<g, 256, 0, st>>>(sp, args.active, args.U, args.F);
      E_(K_COMBINE);
    };
    const dim3 grid(strips * args.U * args.B);
    // StateInit, one launch per m (Var-IO), by the whole-column kernel (2A = 8: weights staged once per
    // workgroup) where the schedule gives it the stage, else by the strip kernel
    bool col_init = false;
    if constexpr (std::is_same<P, P16>::value)
      col_init = (update_rr & kSchedColInit) && col_init_applicable(args);
    B_(col_init ? K_INIT_COL : K_INIT);
    for (int m = 0; m < args.num_init; ++m) {
      plan_stage(bp, args, W, num_it, m, TAIL_READOUT);
      bp.order_rev = launch_no++ & 1;
      if (col_init) {
        if constexpr (std::is_same<P, P16>::value) {
          const hipError_t e = launch_init_col(bp, st);
          if (e != hipSuccess) return e;
        }
        continue;
      }
      stamp_select(-1 - m, st);
      const bool tl = bp.tail == TAIL_AGG;
      const int a2p = init_a2p(args.A);
      if (a2p == 8) launch_init<8>(grid, L, st, bp, tl);
      else if (a2p == 16) launch_init<16>(grid, L, st, bp, tl);
      else launch_init<32>(grid, L, st, bp, tl);
    }
    E_(col_init ? K_INIT_COL : K_INIT);
    combine(bp.a.a_out);
    for (int i = 0; i < num_it; ++i) {
      const bool last = i == num_it - 1;
      plan_stage(bp, args, W, num_it, args.num_init + i, TAIL_READOUT);
      bp.order_rev = launch_no++ & 1;
      bool rr = false, col = false;
      if constexpr (std::is_same<P, P16>::value) {
        col = (update_rr & (last ? kSchedColRo : kSchedColAgg)) && update_col_applicable(args, bp.gz != 0, last, update_rr);
        rr = !col && (update_rr & (last ? kSchedRrRo : kSchedRrAgg)) &&
             update_rr_applicable(args, bp.gz != 0, bp.inline_combine != 0, last);
      }
      const int kid = col ? K_UPDATE_COL : rr ? K_UPDATE_RR : K_UPDATE;
      B_(kid);
      stamp_select(i, st);
      if (col) {
        // whole-column update stage: 48-position items, weights staged once per workgroup
        if constexpr (std::is_same<P, P16>::value) {
          const hipError_t e = launch_update_col(bp, last, st);
          if (e != hipSuccess) return e;
        }
      } else if (rr) {
        // register-resident update stage: 16-row strips, weights staged once per workgroup
        if constexpr (std::is_same<P, P16>::value) {
          const hipError_t e = launch_update_rr(bp, last, st);
          if (e != hipSuccess) return e;
        }
      } else if (last) {
        // paired readout items (heads staged into WB) under the same conditions as the
        // aggregation pairing below, for one LLR head that fits WB
        bool pair_ro = false;
        if constexpr (P::WLDS) {
          const int items = (int)grid.x;
          pair_ro = NRX_PAIR != 0 && NRX_ZDMA != 0 && NRX_PAIR_RO != 0 && args.U <= 2 && bp.inline_combine &&
                    items % 16 == 0 && items >= 2 * cu_count() && args.H == 1 &&
                    heads_fit_wb(args.bits_max, ch32 ? 32 : 16, 2 * args.A);
          if (pair_ro) {
            constexpr int L_wb = strip_lds_bytes<P>(true);
            bp.pair = 1;
            const dim3 g2(items / 2);
            if (ch32) k_update<P, 32, TAIL_READOUT_WB><<<g2, 512, L_wb, st>>>(bp);
            else k_update<P, 16, TAIL_READOUT_WB><<<g2, 512, L_wb, st>>>(bp);
            bp.pair = 0;
          }
        }
        if (!pair_ro) {
          if (ch32) k_update<P, 32, TAIL_READOUT><<<grid, 512, L, st>>>(bp);
          else k_update<P, 16, TAIL_READOUT><<<grid, 512, L, st>>>(bp);
        }
      } else {
        // two items per workgroup when there are at least two per CU (CU count of the
        // device, one workgroup per CU by LDS) and the halves keep the XCD grouping of
        // work_item (items % 16 == 0)
        const int items = (int)grid.x;
        bp.pair = P::WLDS && NRX_PAIR != 0 && NRX_ZDMA != 0 && args.U <= 2 && bp.inline_combine &&
                  items % 16 == 0 && items >= 2 * cu_count();
        const dim3 g2(bp.pair ? items / 2 : items);
        if (ch32) k_update<P, 32, TAIL_AGG><<<g2, 512, L, st>>>(bp);
        else k_update<P, 16, TAIL_AGG><<<g2, 512, L, st>>>(bp);
        bp.pair = 0;
      }
      E_(kid);
      if (!last) combine(bp.a.a_out);
    }
    return hipGetLastError();
  }
};

#ifndef NRX_SMALL_STRIPS
#define NRX_SMALL_STRIPS 1
#endif
// Small grids: the forward is latency-bound and a workgroup's time scales with its rows, so
// the narrowest strips whose items all get a CU of their own are taken (24-row strips
// otherwise).  The readout heads must fit the strip image (X layout: H LLR heads + ChEst,
// 25 KB each).
template <class P>
static bool small_strips_fit(const FwdArgs<_Float16, float, _Float16>& a) {
  const long items = (long)a.B * a.U * ((a.F + P::FO - 1) / P::FO);
  return items <= cu_count() && (a.H + 1) * (kHeadSlot + 1024) <= strip_slots<P>() * slot_pitch<P>();
}
// XCDs (XCCs) of the current device, queried once per device: k_forward keeps one work
// queue per XCD and needs every XCD to hold the same number of CUs (ADVICE r03: 32 per XCD
// was assumed)
static int g_xcc_count[kMaxDevices];
static int xcc_count() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
  if (g_xcc_count[dev] <= 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeNumberOfXccs, dev) != hipSuccess || n <= 0) n = -1;
    g_xcc_count[dev] = n;
  }
  return g_xcc_count[dev];
}

// k_forward covers: U <= 8 (with a workspace under 1 GB conv1 reads z from memory, GZ;
// otherwise the z image is staged in LDS), 1..M StateInit stages (Var-IO), up to three LLR heads,
// 2A <= 32, num_init + num_it <= kFusedMaxStages; 24-row strips with at least two items per
// CU (the small-grid tiers keep the three launches: through k_forward they were slower for
// batch-1 latency, profiles/r03/ab_fused_small_latency.txt); a device whose XCDs hold equal CU
// counts (1..8 XCDs, the queue is picked by the hardware XCC id).  U = 3..8: a combine stage
// (k_combine's f32 pass, one item per (slot, strip)) before each update, whose conv1 then
// reads the combined a_u plane.
// one LLR head whose readout fits the paired-readout WB layout (TAIL_READOUT_WB)
template <class P>
static bool heads_in_wb(const FwdArgs<_Float16, float, _Float16>& a) {
  const int chp = 2 * a.A <= 16 ? 16 : 32;
  return a.H == 1 && heads_fit_wb(a.bits_max, chp, 2 * a.A) &&
         strip_slots<P>() * slot_pitch<P>() + kHW2 + 256 * (a.bits_max + chp) <= fused_lds<P>();
}

template <class P>
static bool fused_gz(const FwdArgs<_Float16, float, _Float16>& a) {
  return a.ws_bytes < kGzOob && a.pe16;
}
template <class P>
static int fused_mode(const FwdArgs<_Float16, float, _Float16>& a) {
  // U > kInlineUsers: combine stages, which the general kernels run
  return !fused_gz<P>(a) ? 2 : (a.num_init > 1 || !heads_in_wb<P>(a) || a.U > kInlineUsers ? 1 : 0);
}

template <class P>
static bool fused_applicable(const FwdArgs<_Float16, float, _Float16>& a, int num_it, const FusedCtl& fc) {
  if (!fc.sync || !fc.enabled) return false;
  const int cus = cu_count(), nx = xcc_count();
  if (nx < 1 || nx > 8 || cus % nx != 0) return false;
  const long items = (long)a.B * a.U * ((a.F + P::FO - 1) / P::FO);
  // readout heads: one LLR head in WB (TAIL_READOUT_WB), or up to three + ChEst in the strip
  // image (TAIL_READOUT, X layout)
  const bool heads = heads_in_wb<P>(a) || (a.H <= 3 && (a.H + 1) * (kHeadSlot + 1024) <= strip_slots<P>() * slot_pitch<P>());
  const int nls = a.num_init + num_it * (a.U > kInlineUsers ? 2 : 1);
  // the default (enabled == 1) takes the GZ schedules (MODE 0, 1) with at least four stages
  // (cfg4, cfg4'): the staged-z kernel (cfg3, cfg5) and the three-stage bench forward (cfg2)
  // measured slower than the three launches on most boxes (DESIGN.md section A.12,
  // profiles/r04/ab_cfg2_fused_vs_three.txt)
  if (fc.enabled == 1 && (fused_mode<P>(a) == 2 || a.num_init + num_it < 4 || a.U > 2)) return false;
  // ... and not where the three column launches apply: they measured faster than k_forward at
  // every shape both run (cfg2 / cfg4 / cfg4', profiles/r06/configs)
  if (fc.enabled == 1 && (fc.update_rr & kSchedColAgg) && fused_gz<P>(a) &&
      update_col_applicable(a, true, false, fc.update_rr))
    return false;
  return items >= 2L * cus && a.U <= kFusedMaxUsers && a.num_init + num_it <= kFusedMaxStages &&
         nls <= kFusedMaxLS && 2 * a.A <= 32 && a.B <= kFusedMaxB && a.bits_max <= 16 && heads;
}

template <class P>
static hipError_t run_fused(const FwdArgs<_Float16, float, _Float16>& args, const ModelW<_Float16, float>& W,
                            int num_it, hipStream_t st, Prof* prof, const FusedCtl& fc) {
  FusedParams<P> fp{};
  fp.sync = reinterpret_cast<FusedSync*>(fc.sync);
  fp.ninit = args.num_init;
  fp.nst = args.num_init + num_it;
  fp.heads_x = !heads_in_wb<P>(args);
  fp.gz = fused_gz<P>(args);
  const bool comb = args.U > kInlineUsers;
  fp.nls = 0;
  for (int s = 0; s < fp.ninit; ++s) {
    fp.kind[fp.nls] = 0;
    fp.pidx[fp.nls++] = s;
  }
  for (int i = 0; i < num_it; ++i) {
    if (comb) {
      fp.kind[fp.nls] = 2;
      fp.pidx[fp.nls++] = fp.ninit + i;
    }
    fp.kind[fp.nls] = 1;
    fp.pidx[fp.nls++] = fp.ninit + i;
  }
  const int cus = cu_count();
  fp.nq = xcc_count();
  fp.spin_limit = fc.spin_limit;
  fp.dbg_err = fc.dbg_err;
  const bool norm_pre = norm_prepass(args, st, prof);
  for (int s = 0; s < fp.nst; ++s) {
    BlockParams<P>& bp = fp.st[s];   // in place: FusedParams is several KB (pair, order_rev, gz stay 0)
    plan_stage(bp, args, W, num_it, s, fp.heads_x ? TAIL_READOUT : TAIL_READOUT_WB);
    bp.inline_combine = comb ? 0 : 1;   // U > 2: the combine stages write a_u in place
    bp.norm_pre = norm_pre;
    bp.strips = (args.F + P::FO - 1) / P::FO;
  }
#ifdef NRX_STAMPS
  {
    const int on = getenv("NRX_STAMP_FUSED") ? 100 : 0;
    (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_nrx_stamp_on), &on, sizeof(int), 0, hipMemcpyHostToDevice, st);
    (void)hipStreamSynchronize(st);
  }
#endif
  if (prof) prof->begin(K_FUSED, st);
  const int a2p = init_a2p(args.A);
  const int mode0 = fused_mode<P>(args);
  const int mode = a2p == 32 && mode0 == 0 ? 1 : mode0;   // 2A = 32 has the general kernels only
  hipError_t e = mode == 0 ? launch_kforward_m0(a2p, fp, cus, st)
                 : mode == 1 ? launch_kforward_m1(a2p, fp, cus, st)
                             : launch_kforward_m2(a2p, fp, cus, st);
  if (e != hipSuccess) return e;
  if (prof) prof->end(K_FUSED, st);
  return hipGetLastError();
}

}  // namespace nrx
