// nrx_dispatch.hip -- plan_forward: which kernel runs each stage of a forward (strip tier, one-launch
// forward or the three launches), on what grid; the one-launch forward's status word, kernel attribute setup.  The
// kernels themselves live in the per-tier translation units nrx_k_*.hip.
#include "nrx_device.inc"
#include "nrx_launch.inc"

namespace nrx {

#ifndef NRX_SMALL_STRIPS
#define NRX_SMALL_STRIPS 1
#endif
// Path `path` with strip stages of tier P for every stage of the forward: the plan of the P16S / P16M / P64 tiers as
// it stands, the base of the 24-row tier's and of k_forward's.
template <class P, class A>
static FwdPlan& plan_strips(FwdPlan& pl, int path, const A& a, int cus) {
  pl.path = path;
  const int strips = (a.F + P::FO - 1) / P::FO, items = strips * a.U * a.B;
  // two items per workgroup when there are at least two per CU (one workgroup per CU by LDS) and the halves
  // keep the XCD grouping of work_item (items % 16 == 0)
  const bool pair = P::WLDS && NRX_PAIR != 0 && NRX_ZDMA != 0 && a.U <= 2 && pl.inline_combine && items % 16 == 0 &&
                    items >= 2 * cus;
  const int chp = 2 * a.A > 16 ? 32 : 16;
  for (int s = 0; s < pl.num_init + pl.num_it; ++s) {
    StagePlan& sp = pl.st[s];
    sp = StagePlan{STAGE_STRIP, K_UPDATE, TAIL_AGG, chp, 0, 0, items, strips, items, strip_lds_bytes<P>(), s & 1};
    if (s < pl.num_init) {
      sp.kid = K_INIT, sp.chp = init_a2p(a.A), sp.tail = s == pl.num_init - 1 ? TAIL_AGG : TAIL_NONE;
    } else if (s < pl.num_init + pl.num_it - 1) {
      sp.pair = pair;
    } else if (pair && NRX_PAIR_RO != 0 && a.H == 1 && heads_fit_wb(a.bits_max, chp, 2 * a.A)) {
      // paired readout items (heads staged into WB), for one LLR head that fits WB
      sp.pair = 1, sp.tail = TAIL_READOUT_WB, sp.lds = strip_lds_bytes<P>(true);
    } else {
      sp.tail = TAIL_READOUT;
    }
    if (sp.pair) sp.grid = items / 2;
  }
  return pl;
}

template <class A>
static FwdPlan plan_base(const A& a, int num_it) {
  FwdPlan pl{};
  pl.num_init = a.num_init, pl.num_it = num_it;
  pl.norm_pre = a.F * kT * 2 * a.A / 4 > kNormFusedMaxQ;
  pl.inline_combine = a.U <= kInlineUsers;
  return pl;
}

FwdPlan plan_forward(const FwdArgs<double, double, float>& a, int num_it) {
  FwdPlan pl = plan_base(a, num_it);
  return plan_strips<P64>(pl, PATH_P64, a, 0);
}

// The f16 forward.  In order: the narrowest strips whose items all get a CU of their own (small
// grids are latency-bound); k_fwd_col; k_forward; the three launches, each stage by the column, RR or strip kernel.
FwdPlan plan_forward(const FwdArgs<_Float16, float, _Float16>& a, int num_it, const Sched& sc, int cus, int xccs) {
  FwdPlan pl = plan_base(a, num_it);
  const int a2 = 2 * a.A, chp = a2 <= 16 ? 16 : 32, nst = a.num_init + num_it;
  // small tiers: the readout heads must fit the strip image (X layout: H LLR heads + ChEst, 25 KB each)
  auto small_fit = [&](int fo, int image) {
    return (long)a.B * a.U * ((a.F + fo - 1) / fo) <= cus && (a.H + 1) * (kHeadSlot + 1024) <= image;
  };
  if (NRX_SMALL_STRIPS != 0 && sc.small && small_fit(P16S::FO, strip_slots<P16S>() * slot_pitch<P16S>()))
    return plan_strips<P16S>(pl, PATH_P16S, a, cus);
  if (NRX_SMALL_STRIPS != 0 && sc.small && small_fit(P16M::FO, strip_slots<P16M>() * slot_pitch<P16M>()))
    return plan_strips<P16M>(pl, PATH_P16M, a, cus);
  constexpr int image = strip_slots<P16>() * slot_pitch<P16>();
  // conv1 can read [a | s | pe] from memory (GZ): the workspace within its 32-bit offsets
  const bool gz_ok = a.ws_bytes < kGzOob && a.pe16 != nullptr;
  // one LLR head whose readout fits the exchange rows of the RR / column kernels
  const bool rr_ro = a.H == 1 && rr_heads_fit(a.bits_max, chp, a2);
  const int cstrips = col_strips(a.F);
  // a column StateInit: 4 rx antennas (2A = A2P = 8: z chunk 0 = [y | h | pe | 0])
  const bool col_init = a2 == 8 && a.init_cinp == 32;
  // a column update, given GZ: a grid wider than one column only with kSchedColWide (44-output strips measured
  // slower than the RR launch at cfg3 / cfg5)
  auto col_update = [&](bool gz, bool last) {
    return (sc.mask & (last ? kSchedColRo : kSchedColAgg)) && gz && a2 <= 32 &&
           (cstrips == 1 || (sc.mask & kSchedColWide)) && (!last || rr_ro);
  };
  // the one-launch paths keep one work queue per XCD and need every XCD to hold the same number of CUs
  const bool queues = sc.fused != 0 && xccs >= 1 && xccs <= 8 && cus % xccs == 0;
  pl.nq = xccs, pl.grid = cus, pl.a2p = init_a2p(a.A);

  // k_fwd_col: U <= 2 (no combine stage), one StateInit over 2A = 8, GZ, one LLR head whose readout fits, at most
  // one item per CU and stage (every item stages its weights)
  if (queues && (sc.mask & kSchedColFwd) && a.U <= kInlineUsers && a.num_init == 1 && col_init && gz_ok && a.H == 1 &&
      rr_heads_fit(a.bits_max, 16, a2) && (long)a.B * a.U * cstrips <= cus && num_it >= 1 &&
      1 + num_it <= kColMaxStages && a.B <= kFusedMaxB) {
    pl.path = PATH_FWD_COL;
    pl.gz = 1, pl.lds = kColLds;
    for (int s = 0; s < nst; ++s) {
      const int tail = s < nst - 1 ? TAIL_AGG : TAIL_READOUT_WB;
      pl.st[s] = StagePlan{STAGE_COL, K_FWD_COL, tail, s == 0 ? 8 : 16, 0, 0, a.B * a.U * cstrips, cstrips, 0, 0, 0};
    }
    return pl;
  }

  // k_forward: 24-row strips, at least two items per CU; the readout heads in WB (one LLR head) or up to three + ChEst
  // in the strip image.  MODE 2 stages the z image in LDS where GZ cannot read it, MODE 1 is the general GZ kernel
  // (combine stages, Var-IO, heads in the strip image, 2A = 32), MODE 0 the bench type.  By default (fused == 1) only
  // GZ schedules of at least four stages and U <= 2 (the others measured slower than the three
  // launches), and not where the column launches take the aggregation updates (faster wherever both run).
  const bool heads_wb = a.H == 1 && heads_fit_wb(a.bits_max, chp, a2) &&
                        image + kHW2 + 256 * (a.bits_max + chp) <= fused_lds<P16>();
  const int mode = !gz_ok ? 2 : (a.num_init > 1 || !heads_wb || !pl.inline_combine || pl.a2p == 32 ? 1 : 0);
  const bool by_default = mode != 2 && nst >= 4 && a.U <= 2 && !col_update(gz_ok, false);
  const int nls = a.num_init + num_it * (pl.inline_combine ? 1 : 2);   // logical stages: a combine stage per update
  if (queues && (sc.fused == 2 || by_default) && (long)a.B * a.U * ((a.F + P16::FO - 1) / P16::FO) >= 2L * cus &&
      a.U <= kFusedMaxUsers && nst <= kFusedMaxStages && nls <= kFusedMaxLS && a2 <= 32 && a.B <= kFusedMaxB &&
      a.bits_max <= 16 && (heads_wb || (a.H <= 3 && (a.H + 1) * (kHeadSlot + 1024) <= image))) {
    plan_strips<P16>(pl, PATH_KFWD0 + mode, a, cus);
    pl.gz = gz_ok, pl.heads_x = !heads_wb, pl.lds = fused_lds<P16>();
    for (int s = 0; s < nst; ++s) {
      StagePlan& sp = pl.st[s];
      sp.kid = K_FUSED, sp.pair = 0, sp.order_rev = 0, sp.grid = 0, sp.lds = 0;
      if (s == nst - 1) sp.tail = heads_wb ? TAIL_READOUT_WB : TAIL_READOUT;
    }
    return pl;
  }

  // the three launches: strip stages, and the column or RR launch for the stages the mask gives them
  plan_strips<P16>(pl, PATH_P16, a, cus);
  pl.gz = NRX_UPDATE_GZ != 0 && gz_ok;
  for (int s = 0; s < nst; ++s) {
    StagePlan& sp = pl.st[s];
    const bool init = s < a.num_init, last = s == nst - 1;
    const bool col = init ? (sc.mask & kSchedColInit) && col_init : col_update(pl.gz, last);
    const bool rr = !init && !col && (sc.mask & (last ? kSchedRrRo : kSchedRrAgg)) && pl.gz && a2 <= 32 &&
                    (!last || rr_ro);
    if (!col && !rr) continue;
    sp.kind = col ? STAGE_COL : STAGE_RR;
    sp.kid = init ? K_INIT_COL : col ? K_UPDATE_COL : K_UPDATE_RR;
    if (last) sp.tail = TAIL_READOUT_WB;
    sp.pair = 0;
    sp.strips = col ? cstrips : (a.F + kRrFO - 1) / kRrFO;
    sp.items = a.B * a.U * sp.strips;
    // a persistent workgroup per CU loops over the items (column kernels: a variant for one item each)
    sp.grid = sp.items < cus ? sp.items : cus;
    sp.one = col && sp.items <= sp.grid;
    sp.lds = col ? kColLds : kRrLds;
    // The lean variants of the one-item column kernels: every launch-uniform fact they hold as a constant (ColLean,
    // nrx_geom.h).  One strip; the slot norm fused; a model with h_hat; one StateInit (masking, or one MCS: its weight
    // is 1 unless a single-MCS mask says otherwise, which the kernel checks once per item); one LLR head of bits_max = 4; 2A = 8 (CHP = 16).  The readout without h_ref
    // is a variant of its own; the other stages ignore h_ref.
    const bool lean = NRX_COL_LEAN != 0 && sp.one && cstrips == 1 && !pl.norm_pre && a.use_h && a.num_init == 1 &&
                      (a.masking || a.M == 1) && a.H == 1 && a.bits_max == 4 && a2 == 8;
    if (col && lean) sp.variant = last && !a.h_ref ? COL_LEAN_NO_HREF : COL_LEAN;
  }
  return pl;
}

hipError_t launch_forward_f16(const Args16& args, const Model16& W, const FwdPlan& pl, const FusedCtl& fc,
                              hipStream_t st, Prof* prof) {
  switch (pl.path) {
    case PATH_P16S: return run_tier_p16s(args, W, pl, st, prof);
    case PATH_P16M: return run_tier_p16m(args, W, pl, st, prof);
    case PATH_FWD_COL: return launch_fwd_col(args, W, pl, fc, st, prof);
    case PATH_P16: return run_tier_p16(args, W, pl, st, prof);
    default: return run_fused<P16>(args, W, pl, fc, st, prof);
  }
}

// CUs and XCDs (XCCs) of the current device, queried once per device: the one cache, read per
// forward by nrx_api.cpp for plan_forward.  A failed query reads as 256 CUs and no XCD count (no one-launch path).
void device_counts(int* cus, int* xccs) {
  constexpr int kMaxDevices = 64;
  static int g_cus[kMaxDevices], g_xccs[kMaxDevices];
  int dev = 0;
  *cus = 256, *xccs = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return;
  if (g_cus[dev] <= 0) {
    int n = 0, x = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return;
    if (hipDeviceGetAttribute(&x, hipDeviceAttributeNumberOfXccs, dev) != hipSuccess || x <= 0) x = -1;
    g_cus[dev] = n, g_xccs[dev] = x;
  }
  *cus = g_cus[dev], *xccs = g_xccs[dev];
}

size_t fused_sync_bytes() { return kFusedSyncBytes; }

// {error word, items that waited, polls} of the fused forward since the last reset.  Blocking:
// the handle's event recorded behind its last one-launch forward is waited for first (ADVICE r04:
// an event the handle owns, never the caller's stream, which may have been destroyed since), so
// the read and the reset never race with a k_forward in flight; reset clears the three words.
hipError_t fused_sync_status(void* sync, int* st, bool reset, hipEvent_t last) {
  FusedSync* sy = reinterpret_cast<FusedSync*>(sync);
  hipError_t e = last ? hipEventSynchronize(last) : hipSuccess;
  if (e == hipSuccess) e = hipMemcpy(st, &sy->err, 3 * sizeof(int), hipMemcpyDeviceToHost);
  if (e == hipSuccess && reset) e = hipMemset(&sy->err, 0, 3 * sizeof(int));
  if (e == hipSuccess && reset) e = hipDeviceSynchronize();
  return e;
}

hipError_t setup_kernels() {
  int cus, xccs;
  device_counts(&cus, &xccs);
  const hipError_t es[] = {setup_tier_p16(),     setup_tier_p16m(),    setup_tier_p16s(),   setup_tier_p64(),
                           setup_kforward_m0(), setup_kforward_m1(), setup_kforward_m2(), setup_update_rr(),
                           setup_col()};
  for (hipError_t e : es)
    if (e != hipSuccess) return e;
  return hipSuccess;
}

int strip_width(int precision) { return precision == 0 ? P16::FO : P64::FO; }

// Device probe of the buffer range check the GZ z-row loader relies on (tests only): one
// raw_buffer_load_dword per lane through a descriptor of `records` bytes at `base`, with the
// lane offset voff + 4 lane in voffset and `soff` in soffset.  Out-of-range loads return 0.  The
// caller keeps base + voff + soff + 256 inside its own allocation, so no outcome can fault.
static __global__ void k_probe_buffer_oob(const char* base, unsigned records, unsigned voff, unsigned soff,
                                          unsigned* out) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), 0, (int)records,
                                                                     0x00020000);
  out[threadIdx.x] = __builtin_amdgcn_raw_buffer_load_b32(r, voff + 4u * threadIdx.x, (int)soff, 0);
}

}  // namespace nrx

extern "C" int nrx_probe_buffer_oob(const void* base, uint32_t records, uint32_t voff, uint32_t soff, uint32_t* out,
                                    void* stream) {
  nrx::k_probe_buffer_oob<<<1, 64, 0, (hipStream_t)stream>>>((const char*)base, records, voff, soff, out);
  return (int)hipGetLastError();
}
