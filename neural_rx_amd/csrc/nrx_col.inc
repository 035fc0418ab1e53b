// nrx_col.inc -- whole-column register-resident launches (k_init_col, k_update_col), f16.
//
// Same math, same HBM layout and bit-identical outputs to the strip kernels (StateInit,
// copy_pytorch.py:160-188; UpdateState :267-287; AggregateUserStates / readouts fused into the
// conv3 epilogue, neural_rx.py:135-207, 309-404); a different item geometry (DESIGN.md section 4):
//
// * One item = one (slot, user, column of 48 subcarrier positions).  The 8 waves own 6
//   consecutive positions each (wave w: positions 6 w .. 6 w + 5), so the two waves of every
//   SIMD carry 12 rows of every layer -- no SIMD imbalance (the RR launch: 5 rows per SIMD for
//   4.5 on average) and, on a grid of at most 48 subcarriers (BASELINE cfg1/2/4: 4 PRB), no halo
//   at all: the whole (slot, user) grid is one item and its edges are the grid's SAME padding.
//   Larger grids run strips of kColFO = 44 outputs (positions 2..45; conv1 reads its z rows from
//   memory, so the halo is 2 rows each side, not 3).
// * Register-resident layer outputs (the RR scheme of nrx_rr.inc): a layer's output stays in the
//   owning wave's registers as the next layer's B fragments; only each wave's first and last rows
//   go through LDS (the exchange rows).  A wave computes its 6 rows in passes of 2 (conv1 /
//   conv2: 8 accumulator tiles per row; conv3: NRX_COL_PR3 = 2 by default, 4 tiles per row), so
//   at most one row more than the 6 own rows is live across a layer.
// * Stage-resident weights: the three layer images (+ the aggregation MLP) are staged into LDS
//   once per workgroup; one workgroup per CU loops over the stage's items (at the bench shape
//   one item per CU).
// * StateInit reads y, h_hat and pe straight from memory into conv1's B fragments (no z
//   image): lane (t, g) of K chunk 0 holds z channels 8 g .. 8 g + 7 = y (g = 0), h_hat (g = 1),
//   pe (g = 2), zero (g = 3) for 2A = 8 (A2P = 8).  The slot norm is the strip kernel's
//   slot_norm (same accumulation order: the same z bits).
// * UpdateState's conv1 reads [a | s | pe] from memory (GZ, struct GZ) as the RR launch does.
//
// Every MFMA sees the operands of the strip kernel's in the same order (bias as the C operand of
// K chunk 0, chunks in order, the same depthwise), so the outputs equal k_init's / k_update's bit
// for bit (tests/test_gpu_col.py).  (Included inside namespace nrx by nrx_k_col.hip, after
// nrx_rr.inc, whose exchange-row helpers it shares.)

#ifndef NRX_COL_PR3
#define NRX_COL_PR3 2
#endif
// (the item geometry kColRO .. kColLds and col_strips: nrx_geom.h)
// subcarrier of position 0, and the positions whose conv3 outputs are valid (one strip: every
// position, the grid edges are the SAME padding; several strips: a 2-row halo each side)
__device__ __forceinline__ int col_fstart(int strip, int strips) { return strips == 1 ? 0 : strip * kColFO - 2; }
__device__ __forceinline__ int col_pos_lo(int strips) { return strips == 1 ? 0 : 2; }
__device__ __forceinline__ int col_pos_hi(int strips) { return strips == 1 ? kColPos : kColPos - 2; }

template <int N, class F, int... I>
__device__ __forceinline__ void col_sfor_(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
// compile-time loop: f(std::integral_constant<int, 0>) .. f(<N - 1>)
template <int N, class F>
__device__ __forceinline__ void col_sfor(F&& f) {
  col_sfor_<N>(f, std::make_integer_sequence<int, N>{});
}

// A separable layer's LDS image (any CINP) with a per-lane bias row (WRr for CINP != 128)
template <int CINP, int COUTP>
struct WCol {
  WLds<P16, CINP, COUTP> w;
  unsigned boff;
  __device__ WCol(const char* base, const char* bias_row, int g) : w{base} {
    boff = rr_lds_addr(bias_row) + 16u * (unsigned)g;
    asm("" : "+v"(boff));
  }
  __device__ half8 afrag(int n, int kc, int lane, int g) const { return w.afrag(n, kc, lane, g); }
  __device__ void dw_taps(int kc, int g, half8 (&t)[9]) const { w.dw_taps(kc, g, t); }
  __device__ floatx4 bias_acc(int n, int) const { return *(rr_lds_cfloatx4*)((rr_lds_cchar*)(size_t)boff + 64 * n); }
};

// Output rows [A, B) of the wave's RO own rows, all COUTP channels, bias included.  Input row i
// (i = -1 .. RO) of K chunk kc is in[i + 1][kc] when REGH (the array holds rows -1 .. RO: conv1 of
// StateInit, whose z rows come from memory), else in[i][kc] for 0 <= i < RO and the neighbours'
// exchange rows (nb) for i = -1 / RO.  Taps and exchange rows of chunk kc + 1 are read once chunk
// kc's depthwise is done; every A fragment is reused over the B - A rows (rr_pass's order).
template <int NKC, int RO, int A, int B, int COUTP, bool REGH, int NIN, class WS>
__device__ __forceinline__ void col_pass(const half8 (&in)[NIN][NKC], const RrNb& nb, const WS& ws, int lane, int g,
                                         floatx4 (&acc)[B - A][COUTP / 16]) {
  constexpr int NR = B - A;
  constexpr int NT = COUTP / 16;
  constexpr bool TOP = !REGH && A == 0, BOT = !REGH && B == RO;
  static_assert(NR >= 1 && A >= 0 && B <= RO && NIN == (REGH ? RO + 2 : RO), "rows");
  half8 w[9], xt{}, xb{};
  auto load = [&](int kc) {
    if constexpr (TOP) xt = rr_ld(nb.top, kc);
    if constexpr (BOT) xb = rr_ld(nb.bot, kc);
    ws.dw_taps(kc, g, w);
  };
  load(0);
#pragma unroll
  for (int kc = 0; kc < NKC; ++kc) {
    half8 a_cur = ws.afrag(0, kc, lane, g);
    half8 d[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = A + r;
      if constexpr (REGH) {
        d[r] = P16::dw_row(in[i][kc], in[i + 1][kc], in[i + 2][kc], w);
      } else {
        const half8 x0 = i - 1 < 0 ? xt : in[i - 1 < 0 ? 0 : i - 1][kc];
        const half8 x2 = i + 1 >= RO ? xb : in[i + 1 >= RO ? RO - 1 : i + 1][kc];
        d[r] = P16::dw_row(x0, in[i][kc], x2, w);
      }
    }
    dw_fence<NR>(d);
    if (kc + 1 < NKC) load(kc + 1);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      half8 a_nxt = a_cur;
      if (n + 1 < NT) a_nxt = ws.afrag(n + 1, kc, lane, g);
      if (kc == 0) {
        const floatx4 bn = ws.bias_acc(n, g);
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r][n] = P16::mma_v(a_cur, d[r], bn);
      } else {
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r][n] = P16::mma_v(a_cur, d[r], acc[r][n]);
      }
      a_cur = a_nxt;
    }
  }
}

// A 128-output layer (conv1 of StateInit from registers, conv2) over the RO own rows in passes
// of PR rows into out[] (ReLU, rows outside the grid zero).  out may not alias in: the caller
// renames (own = out) afterwards, and the compiler keeps an input row only until its last pass.
struct ColNoPost {
  __device__ void operator()() const {}
};
template <int NKC, int RO, int PR, bool REGH, int NIN, class WS, class Post = ColNoPost>
__device__ __forceinline__ void col_layer(const half8 (&in)[NIN][NKC], const RrNb& nb, const WS& ws, int lane, int g,
                                          half8 (&out)[RO][4], int f_own0, int F, Post post0 = Post{}) {
  static_assert(RO % PR == 0, "passes");
  col_sfor<RO / PR>([&](auto J) __attribute__((always_inline)) {
    constexpr int A = decltype(J)::value * PR;
    floatx4 acc[PR][8];
    col_pass<NKC, RO, A, A + PR, kHID, REGH>(in, nb, ws, lane, g, acc);
    rr_to_own<RO, A, A + PR>(acc, out, f_own0, F);
    if constexpr (A == 0) post0();   // after the first pass (the deferred weight stores)
  });
}

// conv1 of UpdateState: z rows [a | s | pe] from memory (GZ), passes of PR rows.  A step is one
// (pass j, K chunk kc): the depthwise of its PR + 2 input rows, then its 8 x PR MFMAs.  The rows of
// step s + NRX_COL_ZD are loaded once step s's depthwise is done (a ring of NRX_COL_ZD buffers):
// one step is ~500 cycles of a wave, an L2 / MALL round trip longer, and a 1-step lookahead left
// conv1 twice its math time (profiles/r06 stamps).  z holds steps 0 .. ZD - 1 on entry (issued by
// the caller before its barrier).
#ifndef NRX_COL_ZD
#define NRX_COL_ZD 2
#endif
// diagnostic builds (NRX_STAMPS + NRX_PRO_STAMPS): stamps inside the first item's prologue and
// conv1, in the item-1 slots a one-item launch leaves free (tools/stamps_col.py NRX_PRO=1)
#if defined(NRX_STAMPS) && defined(NRX_PRO_STAMPS)
#define COL_PRO_TS(m) rr_ts(1, m)
#else
#define COL_PRO_TS(m)
#endif
template <int PR>
struct ColZ {
  static constexpr int D = NRX_COL_ZD;
  unsigned soff[kColRO + 2];
  half8 xb[D][PR + 2];
};
template <int PR>
__device__ __forceinline__ void col_gz_load_step(ColZ<PR>& z, const GZ& gz, int s) {
  const int j = s / 4, kc = s % 4;
#pragma unroll
  for (int i = 0; i < PR + 2; ++i) z.xb[s % ColZ<PR>::D][i] = gz.load(kc, z.soff[j * PR + i]);
}
template <int PR>
__device__ __forceinline__ void col_gz_first(ColZ<PR>& z, const GZ& gz, int p0) {
#pragma unroll
  for (int i = 0; i < kColRO + 2; ++i) z.soff[i] = gz.row_soff(p0 - 1 + i);
#pragma unroll
  for (int s = 0; s < ColZ<PR>::D; ++s) col_gz_load_step<PR>(z, gz, s);
}
template <int PR, class WS, class Post = ColNoPost>
__device__ __forceinline__ void col_conv1_gz(ColZ<PR>& z, const GZ& gz, const WS& ws, int lane, int g,
                                             half8 (&out)[kColRO][4], int f_own0, int F, Post post0 = Post{}) {
  constexpr int RO = kColRO, NP = RO / PR, NS = NP * 4, D = ColZ<PR>::D;
  half8 w[9];
  ws.dw_taps(0, g, w);
  col_sfor<NP>([&](auto J) __attribute__((always_inline)) {
    constexpr int j = decltype(J)::value;
    floatx4 acc[PR][8];
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const int s = j * 4 + kc;
      half8 a_cur = ws.afrag(0, kc, lane, g);
      half8 d[PR];
#pragma unroll
      for (int r = 0; r < PR; ++r) d[r] = P16::dw_row(z.xb[s % D][r], z.xb[s % D][r + 1], z.xb[s % D][r + 2], w);
      dw_fence<PR>(d);
      if constexpr (!std::is_same_v<Post, ColNoPost>) {
        if (s == 0) COL_PRO_TS(3);
      }
      // this step's buffer takes step s + D; the next step's taps
      if (s + D < NS) col_gz_load_step<PR>(z, gz, s + D);
      if (s + 1 < NS) ws.dw_taps((kc + 1) % 4, g, w);
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        half8 a_nxt = a_cur;
        if (n + 1 < 8) a_nxt = ws.afrag(n + 1, kc, lane, g);
        if (kc == 0) {
          const floatx4 bn = ws.bias_acc(n, g);
#pragma unroll
          for (int r = 0; r < PR; ++r) acc[r][n] = P16::mma_v(a_cur, d[r], bn);
        } else {
#pragma unroll
          for (int r = 0; r < PR; ++r) acc[r][n] = P16::mma_v(a_cur, d[r], acc[r][n]);
        }
        a_cur = a_nxt;
      }
    }
    rr_to_own<RO, j * PR, (j + 1) * PR>(acc, out, f_own0, F);
    if constexpr (j == 0 && !std::is_same_v<Post, ColNoPost>) {
      COL_PRO_TS(4);
      post0();   // after the first pass (the deferred weight stores)
      COL_PRO_TS(5);
    }
  });
}

// conv3 + the fused epilogue (new state + next aggregation MLP) in passes of PR rows; p0 = the
// position of own row 0.
template <int PR, class Epi>
__device__ __forceinline__ void col_conv3(const half8 (&own)[kColRO][4], const RrNb& nb, Epi& epi, int lane, int t,
                                          int g, int p0) {
  col_sfor<kColRO / PR>([&](auto J) __attribute__((always_inline)) {
    constexpr int A = decltype(J)::value * PR;
    typename Epi::template PrefT<PR> pf;
    epi.template prefetch<PR>(pf, p0 + A, t, g);   // skip-connection rows, in flight during the math
    floatx4 acc[PR][4];
    col_pass<4, kColRO, A, A + PR, kDSP, false>(own, nb, epi.ws, lane, g, acc);
    epi.template settle<PR>(pf);
    epi.template run<PR>(acc, pf, p0 + A, t, g, 0, PR);
  });
}

// Readout variant: conv3 in passes of PR rows, each pass's new-state fragments kept (8 VGPRs a
// row); once every own row is consumed the heads run RB rows at a time (EpiConv3::readout_rows),
// so the heads' hidden layers never share the registers with the own rows.
#ifndef NRX_COL_RB
#define NRX_COL_RB 3
#endif
template <int PR, class Epi>
__device__ __forceinline__ void col_conv3_ro(const half8 (&own)[kColRO][4], const RrNb& nb, Epi& epi, int lane, int t,
                                             int g, int p0) {
  constexpr int RB = NRX_COL_RB;
  static_assert(kColRO % RB == 0, "readout row batches");
  CFrag<P16, kDSP / 16> sb[kColRO];
  bool ok[kColRO];
  col_sfor<kColRO / PR>([&](auto J) __attribute__((always_inline)) {
    constexpr int A = decltype(J)::value * PR;
    typename Epi::template PrefT<PR> pf;
    epi.template prefetch<PR>(pf, p0 + A, t, g);
    floatx4 acc[PR][4];
    col_pass<4, kColRO, A, A + PR, kDSP, false>(own, nb, epi.ws, lane, g, acc);
    epi.template settle<PR>(pf);
    CFrag<P16, kDSP / 16> sbp[PR];
    bool okp[PR];
    epi.template state_frags<PR>(acc, pf, p0 + A, t, g, sbp, okp);
#pragma unroll
    for (int r = 0; r < PR; ++r) {
      sb[A + r] = sbp[r];
      ok[A + r] = okp[r];
    }
  });
  col_sfor<kColRO / RB>([&](auto J) __attribute__((always_inline)) {
    constexpr int A = decltype(J)::value * RB;
    CFrag<P16, kDSP / 16> sbr[RB];
    bool okr[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      sbr[r] = sb[A + r];
      okr[r] = ok[A + r];
    }
    epi.template readout_rows<RB>(sbr, okr, p0 + A, t, g);
  });
}

// Diagnostic builds (NRX_STAMPS): s_memtime of lane 0 of waves 0 and 4 at the phase ends of the
// workgroup's items k < 4 (nrx_rr.inc's layout: m = 0 item start, 1 conv1 math, 2 conv1 rows
// exchanged, 3 conv2 math, 4 conv2 rows exchanged, 5 heads staged (readout), 6 item done).
__device__ __forceinline__ void col_ts(int k, int m) { rr_ts(k, m); }

// The launch's weights: conv1 image (CINP1 inputs), conv2, conv3 (+ the aggregation MLP for
// TAIL_AGG, in the unused half of conv3's W^T region: the strip kernels' WB layout), the -inf and
// zero blocks.  load() issues every global load (~50 VGPRs); the kernels issue the first item's
// own loads behind them and store() once the weights have landed, so the first item's input
// latency hides under the staging instead of following it.
template <int CINP1, int TAILM>
struct ColStage {
  SepStage<CINP1, kHID> s1;
  SepStage<kHID, kHID> s2;
  SepStage<kHID, kDSP> s3;
  DenseStage<kDSP, kAGG> d1;
  DenseStage<kAGG, kDSP> d2;
  // conv1's image first: the item's first loads follow it and the rest of the images after those,
  // so that conv1 waits (vmcnt counts in issue order) for its own image and rows only
  __device__ __forceinline__ void load_w1(const BlockParams<P16>& prm) { s1.load(prm.w[0]); }
  __device__ __forceinline__ void load_rest(const BlockParams<P16>& prm) {
    s2.load(prm.w[1]);
    s3.load(prm.w[2]);
    if constexpr (TAILM == TAIL_AGG) {
      d1.load(prm.agg[0]);
      d2.load(prm.agg[1]);
    }
  }
  __device__ __forceinline__ void load(const BlockParams<P16>& prm) {
    load_w1(prm);
    load_rest(prm);
  }
  // conv1's image and the -inf / zero blocks (before the first barrier) ...
  __device__ __forceinline__ void store_w1(char* smem) const {
    s1.store(smem + kRrW1);
    for (int i = nrx_tid(); i < 768 / 4; i += 512) reinterpret_cast<float*>(smem + kRrNeg)[i] = -__builtin_inff();
    for (int i = nrx_tid(); i < kRrExChunk * 4 / 16; i += 512)
      reinterpret_cast<intx4*>(smem + kRrZero)[i] = intx4{0, 0, 0, 0};
  }
  // ... and the rest once conv1's first pass is done (read from conv2 on, behind the exchange
  // barriers): their load latency hides under that pass instead of before it
  __device__ __forceinline__ void store_rest(char* smem) const {
    s2.store(smem + kRrW2);
    s3.store(smem + kRrW3);
    if constexpr (TAILM == TAIL_AGG) {
      d1.store(smem + kRrW3 + 16 * 1024, reinterpret_cast<float*>(smem + kRrW3 + kWTailBias));
      d2.store(smem + kRrW3 + 24 * 1024, reinterpret_cast<float*>(smem + kRrW3 + kWTailBias + kAGG * 4));
    }
  }
  __device__ __forceinline__ void store(char* smem) const {
    store_w1(smem);
    store_rest(smem);
  }
};

// ------------------------------------------------------------------------ UpdateState
// One item (slot b, user u, strip) on the calling wave.  Every wave runs the same barriers.
// TAIL_AGG: conv3's epilogue writes s' and act*sp.  TAIL_READOUT_WB: once every wave is past
// conv2 the heads are staged over the conv1 / conv2 images (dead for this item; restaged by the
// caller before a next item), and conv3's epilogue runs the readouts.
template <int CHP, int TAILM, bool FIRST = false, class LT = ColGeneric>
__device__ __forceinline__ void col_upd_item(const BlockParams<P16>& prm, char* smem, int wave, int b, int u, int strip,
                                             int k, ColStage<kUPD_CINP, TAILM>* stage = nullptr) {
  constexpr int PR = 2;
  col_ts(k, 0);
  const int lane = nrx_tid() & 63, t = lane & 15, g = lane >> 4;
  const int p0 = kColRO * wave;
  const int strips = prm.strips;   // (lean: 1, read all the same -- as a constant it cost 10 VGPRs of spills)
  const int f_start = col_fstart(strip, strips);
  const int F = prm.a.F;
  const int f_own0 = f_start + p0;
  const RrNb nb = rr_nb(smem, wave, t, g);
  half8 own[kColRO][4];
  const GZ gz = gz_make(prm, b, u, f_start, t, g);
  ColZ<PR> z;
  col_gz_first<PR>(z, gz, p0);
  if constexpr (FIRST) {
    COL_PRO_TS(0);
    stage->load_rest(prm);   // behind conv1's image (caller: load_w1) and first rows
                             // (later issue measured slower: profiles/r06/prologue_stamps_and_rest_late.txt)
    COL_PRO_TS(1);
    stage->store_w1(smem);
    COL_PRO_TS(2);
    __syncthreads();
  }
  col_ts(k, 5);
  {
    const WRr<kHID> w1(smem + kRrW1, t < kT ? smem + kRrW1 + kWBias : smem + kRrNeg + kRrNegOff, g);
    if constexpr (FIRST) col_conv1_gz<PR>(z, gz, w1, lane, g, own, f_own0, F, [&]() { stage->store_rest(smem); });
    else col_conv1_gz<PR>(z, gz, w1, lane, g, own, f_own0, F);
  }
  col_ts(k, 1);
  __syncthreads();   // every wave is past the previous item's reads of X
  rr_write_exch<kColRO>(smem, wave, t, g, own);
  __syncthreads();
  col_ts(k, 2);
  {
    const WRr<kHID> w2(smem + kRrW2, t < kT ? smem + kRrW2 + kWBias : smem + kRrNeg + kRrNegOff, g);
    half8 nxt[kColRO][4];
    col_layer<4, kColRO, PR, false>(own, nb, w2, lane, g, nxt, f_own0, F);
#pragma unroll
    for (int r = 0; r < kColRO; ++r)
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) own[r][kc] = nxt[r][kc];
  }
  col_ts(k, 3);
  using WS3 = WLds<P16, kHID, kDSP>;
  const WS3 w3{smem + kRrW3};
  char* WB = TAILM == TAIL_READOUT_WB ? smem + kRrW1 : smem + kRrW3;
  if constexpr (TAILM == TAIL_READOUT_WB) {
    RrHeads<CHP> hd;
    hd.load(prm);
    __syncthreads();   // every wave is past its conv2 reads (of the conv1 exchange rows and W2)
    rr_write_exch<kColRO>(smem, wave, t, g, own);
    hd.store(WB, prm);
  } else {
    __syncthreads();   // every wave is past its conv2 reads of the conv1 exchange rows
    rr_write_exch<kColRO>(smem, wave, t, g, own);
  }
  __syncthreads();
  col_ts(k, 4);
  EpiConv3<P16, WS3, CHP, TAILM, LT> epi{&prm, nullptr, WB, w3, b, u, f_start, col_pos_hi(strips), 0, 1.f, false,
                                     (float)prm.a.active[(size_t)b * prm.a.U + u], -1, 0, 0};
  epi.pos_lo = col_pos_lo(strips);
  if constexpr (TAILM == TAIL_READOUT_WB) col_conv3_ro<NRX_COL_PR3>(own, nb, epi, lane, t, g, p0);
  else col_conv3<NRX_COL_PR3>(own, nb, epi, lane, t, g, p0);
  col_ts(k, 6);
}

// UpdateState of a whole stage: grid = min(items, CUs), one workgroup per CU (LDS), items
// i = blockIdx.x + k gridDim.x in work_item's XCD-grouped order.  Two kernels: k_update_col runs
// one item per workgroup (items <= CUs: every BASELINE single-column shape), k_update_col_multi
// loops over several.  The loop's code kept thread-derived addresses live across the first item
// and cost that item 22 (readout) / 4 (aggregation) VGPRs of spills; without it the single-item
// kernel spills 4 / 1.
template <int CHP, int TAILM, bool MULTI, class LT = ColGeneric>
__device__ __forceinline__ void col_update_stage(const BlockParams<P16>& prm, int items) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  rr_ts(0, 7);
  rr_ts_edge(0);
  const int wave = __builtin_amdgcn_readfirstlane(nrx_tid() >> 6);
  int k = 0;
  {
    ColStage<kUPD_CINP, TAILM> stage;
    stage.load_w1(prm);
    int b, u, strip;
    work_item(blockIdx.x, prm.a.B, prm.a.U, prm.strips, prm.order_rev, b, u, strip);
    col_upd_item<CHP, TAILM, true, LT>(prm, smem, wave, b, u, strip, k, &stage);   // grid <= items
  }
  if constexpr (MULTI) {
    for (int i = blockIdx.x; i < items; i += gridDim.x, ++k) {
      int b, u, strip;
      if (k > 0) {
        work_item(i, prm.a.B, prm.a.U, prm.strips, prm.order_rev, b, u, strip);
        col_upd_item<CHP, TAILM>(prm, smem, wave, b, u, strip, k);
      }
      if constexpr (TAILM == TAIL_READOUT_WB) {
        if (i + (int)gridDim.x < items) {
          // the heads sit over the conv1 / conv2 images: restage them for the next item
          SepStage<kUPD_CINP, kHID> s1;
          SepStage<kHID, kHID> s2;
          s1.load(prm.w[0]);
          s2.load(prm.w[1]);
          __syncthreads();   // every wave is past its readout epilogue
          s1.store(smem + kRrW1);
          s2.store(smem + kRrW2);
          __syncthreads();
        }
      }
    }
  }
  rr_ts_edge(1);
}

template <int CHP, int TAILM, class LT = ColGeneric>
__global__ __launch_bounds__(512) void k_update_col(BlockParams<P16> prm, int items) {
  col_update_stage<CHP, TAILM, false, LT>(prm, items);
}
template <int CHP, int TAILM>
__global__ __launch_bounds__(512) void k_update_col_multi(BlockParams<P16> prm, int items) {
  col_update_stage<CHP, TAILM, true>(prm, items);
}

// ------------------------------------------------------------------------ StateInit
// z rows of StateInit for 2A = A2P = 8: K chunk 0 of z = [y*ns (8) | h*ns (8) | pe (2) | 0],
// lane (t, g) holding channels 8 g .. 8 g + 7.  Loads from clamped addresses (row 0 / symbol 0
// of the slot: always inside the tensors), masked afterwards.
struct ColInitRow {
  floatx4 v0, v1;   // y (g != 1) or h_hat (g == 1) channels 0..7
  float2 pe;
};
__device__ __forceinline__ ColInitRow col_init_load(const FwdArgs<_Float16, float, _Float16>& a, int b, int u, int f,
                                                    int t, int g) {
  const bool ok = f >= 0 && f < a.F && t < kT;
  const size_t re = ((size_t)b * a.F + (ok ? f : 0)) * kT + (ok ? t : 0);
  const float* src = a.y + re * 8;
  if (g == 1 && a.use_h) src = a.h_hat + ((size_t)b * a.U * a.F * kT + (size_t)u * a.F * kT + (re - (size_t)b * a.F * kT)) * 8;
  ColInitRow r;
  r.v0 = reinterpret_cast<const floatx4*>(src)[0];
  r.v1 = reinterpret_cast<const floatx4*>(src)[1];
  r.pe = *reinterpret_cast<const float2*>(a.pe + (((size_t)u * a.F + (ok ? f : 0)) * kT + (ok ? t : 0)) * 2);
  return r;
}
// the z chunk of one row: the strip kernel's values (f32_rounded(y * ns) -> f16, pe -> f16, zero
// outside the grid, for t >= 14, for h when the model takes no h_hat, and for g = 3)
__device__ __forceinline__ half8 col_init_z(const ColInitRow& r, float ns, bool ok, int g, bool use_h) {
  const float v[8] = {r.v0[0], r.v0[1], r.v0[2], r.v0[3], r.v1[0], r.v1[1], r.v1[2], r.v1[3]};
  half8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float x = f32_rounded(v[e] * ns);
    if (g == 2) x = e == 0 ? r.pe.x : (e == 1 ? r.pe.y : 0.f);
    if (!ok || g == 3 || (g == 1 && !use_h)) x = 0.f;
    o[e] = (_Float16)x;
  }
  return o;
}

// Lean variants (ColLean: one strip, a model with h_hat, 2A = 8): each lane picks its source plane once -- y
// (g != 1) or h_hat (g = 1) of its slot (and user), a 64-bit base -- and a row adds one unsigned 32-bit offset; pe
// goes through a wave-uniform plane base.  Same clamping as col_init_load.
struct ColInitLane {
  const char* src;
  const char* pe;
};
__device__ __forceinline__ ColInitLane col_init_lane(const FwdArgs<_Float16, float, _Float16>& a, int b, int u, int g) {
  const size_t plane = (size_t)a.F * kT * 8;
  const float* y = a.y + (size_t)b * plane;
  const float* h = a.h_hat + ((size_t)b * a.U + u) * plane;
  return ColInitLane{reinterpret_cast<const char*>(g == 1 ? h : y),
                     reinterpret_cast<const char*>(a.pe + (size_t)u * a.F * kT * 2)};
}
__device__ __forceinline__ ColInitRow col_init_load_lean(const ColInitLane& ln, int F, int f, int t) {
  const bool ok = f >= 0 && f < F && t < kT;
  const unsigned re = (unsigned)((ok ? f : 0) * kT + (ok ? t : 0));
  ColInitRow r;
  r.v0 = *reinterpret_cast<const floatx4*>(ln.src + re * 32u);
  r.v1 = *reinterpret_cast<const floatx4*>(ln.src + re * 32u + 16u);
  r.pe = *reinterpret_cast<const float2*>(ln.pe + re * 8u);
  return r;
}
// col_init_z with the source picked per lane group: sc = ns for the y / h_hat lanes (g < 2) and 1 for the pe lanes
// (g = 2: pe * 1 = pe), whose two pe values replace the lane's first two elements; the eight elements are converted
// without selects and the four packed words masked (word 0: g < 3, words 1..3: g < 2; none outside the grid).  The
// values are col_init_z's: f32_rounded(y * ns) -> f16, pe -> f16, zero elsewhere.
__device__ __forceinline__ half8 col_init_z_lean(const ColInitRow& r, float sc, bool ok, int g) {
  float v[8] = {r.v0[0], r.v0[1], r.v0[2], r.v0[3], r.v1[0], r.v1[1], r.v1[2], r.v1[3]};
  if (g == 2) v[0] = r.pe.x, v[1] = r.pe.y;
  half8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (_Float16)f32_rounded(v[e] * sc);
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  u32x4 w = __builtin_bit_cast(u32x4, o);
  const bool k0 = ok && g < 3, k1 = ok && g < 2;
  w[0] = k0 ? w[0] : 0u;
#pragma unroll
  for (int i = 1; i < 4; ++i) w[i] = k1 ? w[i] : 0u;
  return __builtin_bit_cast(half8, w);
}

// One item (slot b, user u, strip) of StateInit m = prm.m on the calling wave (A2P = 8): the state
// is the sum over the launches m of wm * SI_m(z) (Var-IO), and the last launch's TAIL_AGG stores
// act * sp of iteration 0.
template <int TAILM, bool FIRST = false, class LT = ColGeneric>
__device__ __forceinline__ void col_init_item(const BlockParams<P16>& prm, char* smem, int wave, int b, int u,
                                              int strip, int k, ColStage<32, TAILM>* stage = nullptr) {
  constexpr int PR = 2;
  constexpr bool LEAN = LT::kLean;
  col_ts(k, 0);
  const auto& a = prm.a;
  const int lane = nrx_tid() & 63, t = lane & 15, g = lane >> 4;
  const int p0 = kColRO * wave;
  const int strips = LEAN ? 1 : prm.strips;
  const int f_start = col_fstart(strip, strips);
  const int F = a.F, A2 = LEAN ? 8 : 2 * a.A;
  const bool norm_pre = LEAN ? false : prm.norm_pre != 0;
  const int f_own0 = f_start + p0;
  const RrNb nb = rr_nb(smem, wave, t, g);
  // the slot norm's y loads and the wave's z rows (positions p0 - 1 .. p0 + 6) go out together
  const float* yslot = a.y + (size_t)b * F * kT * A2;
  const int nqs = F * kT * A2 / 4;
  NormPre npre;
  if (!norm_pre) npre = slot_norm_issue(yslot, nqs);
  ColInitRow zr[kColRO + 2];
  if constexpr (LEAN) {
    const ColInitLane ln = col_init_lane(a, b, u, g);
#pragma unroll
    for (int i = 0; i < kColRO + 2; ++i) zr[i] = col_init_load_lean(ln, F, f_own0 - 1 + i, t);
  } else {
#pragma unroll
    for (int i = 0; i < kColRO + 2; ++i) zr[i] = col_init_load(a, b, u, f_own0 - 1 + i, t, g);
  }
  if constexpr (FIRST) stage->load_rest(prm);   // behind conv1's image (caller: load_w1), the norm and z rows
  // Var-IO weight of StateInit m (prm.m; masking: one StateInit of weight 1).  The launch of
  // StateInit m > 0 adds its weighted output to the state the earlier ones wrote (EpiConv3 mode 1,
  // first = m == 0), as the strip kernel's launches do; an item of weight 0 runs its math (0 *
  // finite: the same state bits as the strip kernel's skipped item)
  // (lean: the one StateInit, m = 0; its weight is 1 under masking and without a mask)
  const int m = LEAN ? 0 : prm.m;
  // (no mask: one-hot on MCS 0, as the strip kernels take it)
  const float wm = a.masking ? 1.f : (a.mcs_mask ? a.mcs_mask[((size_t)b * a.U + u) * a.M + m] : (m == 0 ? 1.f : 0.f));
  if constexpr (FIRST) {
    stage->store_w1(smem);   // the weights were loaded before the norm / z rows above; slot_norm's
    if (norm_pre) __syncthreads();   // barrier (or this one) publishes them before conv1
  }
  const float ns = norm_pre ? (float)a.norm[b]
                                : (float)slot_norm(npre, yslot, nqs, reinterpret_cast<double*>(smem + kColRed));
  col_ts(k, 5);
  half8 zin[kColRO + 2][1];
  const float zsc = g == 2 ? 1.f : ns;   // (lean) the lane group's scale
#pragma unroll
  for (int i = 0; i < kColRO + 2; ++i) {
    const int f = f_own0 - 1 + i;
    if constexpr (LEAN) zin[i][0] = col_init_z_lean(zr[i], zsc, f >= 0 && f < F && t < kT, g);
    else zin[i][0] = col_init_z(zr[i], ns, f >= 0 && f < F && t < kT, g, a.use_h != 0);
  }
  dpp_in_fence(zin);   // the conversions are VALU writes the depthwise's DPP reads
  // pe16 rows of this item's outputs for the update items' conv1 (every slot writes the same bytes)
  if (a.pe16 && g == 2 && t < kT) {
#pragma unroll
    for (int i = 1; i <= kColRO; ++i) {
      const int p = p0 + i - 1, f = f_start + p;
      if (p >= col_pos_lo(strips) && p < col_pos_hi(strips) && f >= 0 && f < F) {
        const half8 h = zin[i][0];
        *reinterpret_cast<half8*>(a.pe16 + (((size_t)u * F + f) * kT + t) * kDS) = h;
      }
    }
  }
  half8 own[kColRO][4];
  {
    const WCol<32, kHID> w1(smem + kRrW1, t < kT ? smem + kRrW1 + kWBias : smem + kRrNeg + kRrNegOff, g);
    half8 o1[kColRO][4];
    if constexpr (FIRST) col_layer<1, kColRO, PR, true>(zin, nb, w1, lane, g, o1, f_own0, F, [&]() { stage->store_rest(smem); });
    else col_layer<1, kColRO, PR, true>(zin, nb, w1, lane, g, o1, f_own0, F);
#pragma unroll
    for (int r = 0; r < kColRO; ++r)
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) own[r][kc] = o1[r][kc];
  }
  col_ts(k, 1);
  __syncthreads();   // every wave is past the previous item's reads of X
  rr_write_exch<kColRO>(smem, wave, t, g, own);
  __syncthreads();
  col_ts(k, 2);
  {
    const WRr<kHID> w2(smem + kRrW2, t < kT ? smem + kRrW2 + kWBias : smem + kRrNeg + kRrNegOff, g);
    half8 nxt[kColRO][4];
    col_layer<4, kColRO, PR, false>(own, nb, w2, lane, g, nxt, f_own0, F);
#pragma unroll
    for (int r = 0; r < kColRO; ++r)
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) own[r][kc] = nxt[r][kc];
  }
  col_ts(k, 3);
  __syncthreads();   // every wave is past its conv2 reads of the conv1 exchange rows
  rr_write_exch<kColRO>(smem, wave, t, g, own);
  __syncthreads();
  col_ts(k, 4);
  using WS3 = WLds<P16, kHID, kDSP>;
  const WS3 w3{smem + kRrW3};
  EpiConv3<P16, WS3, 16, TAILM, LT> epi{&prm, nullptr, smem + kRrW3, w3, b, u, f_start, col_pos_hi(strips), 1, wm, m == 0,
                                    (float)a.active[(size_t)b * a.U + u], -1, 0, 0};
  epi.pos_lo = col_pos_lo(strips);
  col_conv3<NRX_COL_PR3>(own, nb, epi, lane, t, g, p0);
  col_ts(k, 6);
}

// StateInit of a whole stage; k_init_col (one item per workgroup) / k_init_col_multi as above
template <int TAILM, bool MULTI, class LT = ColGeneric>
__device__ __forceinline__ void col_init_stage(const BlockParams<P16>& prm, int items) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  rr_ts(0, 7);
  rr_ts_edge(0);
  const int wave = __builtin_amdgcn_readfirstlane(nrx_tid() >> 6);
  {
    ColStage<32, TAILM> stage;
    stage.load_w1(prm);
    int b, u, strip;
    work_item(blockIdx.x, prm.a.B, prm.a.U, LT::kLean ? 1 : prm.strips, prm.order_rev, b, u, strip);
    col_init_item<TAILM, true, LT>(prm, smem, wave, b, u, strip, 0, &stage);   // grid <= items
  }
  if constexpr (MULTI) {
    int k = 1;
    for (int i = blockIdx.x + gridDim.x; i < items; i += gridDim.x, ++k) {
      int b, u, strip;
      work_item(i, prm.a.B, prm.a.U, prm.strips, prm.order_rev, b, u, strip);
      col_init_item<TAILM>(prm, smem, wave, b, u, strip, k);
    }
  }
  rr_ts_edge(1);
}

template <int TAILM, class LT = ColGeneric>
__global__ __launch_bounds__(512) void k_init_col(BlockParams<P16> prm, int items) {
  col_init_stage<TAILM, false, LT>(prm, items);
}
template <int TAILM>
__global__ __launch_bounds__(512) void k_init_col_multi(BlockParams<P16> prm, int items) {
  col_init_stage<TAILM, true>(prm, items);
}

// ------------------------------------------------------------------------ one-launch forward
// k_fwd_col: StateInit, the num_it - 1 aggregation updates and the readout update of a forward as
// ONE persistent launch of column items (k_forward's queue discipline, nrx_device.inc): one work
// queue per XCD (the XCC id read from the hardware), holding the items of the slots b with
// b % nq == queue in stage-major order; a workgroup dequeues one item at a time, an item of stage
// s >= 1 waits for its slot's stage s - 1 counter (every item it waits for was dequeued earlier
// by a running workgroup: no deadlock whatever the residency), producer and consumer share the
// XCD's L2 (the consumer invalidates its L1 after the wait, fused_wait).  What it removes from
// the three launches: two launch gaps and two kernel prologues (kernel-argument loads) per
// forward.  Every item stages its stage's weights (the bench shape gives each workgroup one item
// per stage), so it is taken for shapes with at most one item per CU and stage.
struct ColFwdParams {
  BlockParams<P16> st[kColMaxStages];   // 0: StateInit, 1 .. nst - 1: the updates (the last: readouts)
  FusedSync* sync;
  int nst;
  int nq;           // queues (XCDs)
  int spin_limit;   // dependency-wait polls before the timeout error
  int dbg_err;      // debug: error bits workgroup 0 sets (nrx_fused_config inject_err)
};

// One item of k_fwd_col (every item stages its stage's weights): KIND 0 StateInit, 1 an
// aggregation update, 2 the readout update
template <int CHP, int KIND>
__device__ __forceinline__ void fwd_col_item(const BlockParams<P16>& prm, char* smem, int wave, int b, int u,
                                             int strip, int k) {
  if constexpr (KIND == 0) {
    ColStage<32, TAIL_AGG> st;
    st.load_w1(prm);
    col_init_item<TAIL_AGG, true>(prm, smem, wave, b, u, strip, k, &st);
  } else if constexpr (KIND == 1) {
    ColStage<kUPD_CINP, TAIL_AGG> st;
    st.load_w1(prm);
    col_upd_item<CHP, TAIL_AGG, true>(prm, smem, wave, b, u, strip, k, &st);
  } else {
    ColStage<kUPD_CINP, TAIL_READOUT_WB> st;
    st.load_w1(prm);
    col_upd_item<CHP, TAIL_READOUT_WB, true>(prm, smem, wave, b, u, strip, k, &st);
  }
}

// item done: its stores have reached L2 (every wave's vmcnt drained), then one agent-scope add on
// the slot's counter and the next dequeue
__device__ __forceinline__ int fwd_col_done(int* cnt, int* head, int* sh) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (nrx_tid() == 0) {
    __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh[0] = atomicAdd(head, 1);
  }
  __syncthreads();
  return sh[0];
}

#ifdef NRX_STAMPS
// diagnostic: lane 0 of wave 0 after the dependency wait, in the (unused) wave-4 slot of m = 7
#define NRX_FC_WAIT_STAMP(k)                                                  \
  if (nrx_tid() == 0 && g_nrx_stamp_on && (k) < 4 && blockIdx.x < 4096) \
    g_nrx_rr_stamps[blockIdx.x][16 * (k) + 15] = __builtin_amdgcn_s_memtime();
#else
#define NRX_FC_WAIT_STAMP(k)
#endif

template <int CHP>
__global__ __launch_bounds__(512) void k_fwd_col(ColFwdParams fp_arg) {
  // the stage parameters are read through the kernarg segment pointer (k_forward: indexing the
  // by-value parameter with a dynamic stage copied the whole struct to scratch)
  typedef const __attribute__((address_space(4))) ColFwdParams KFP;
  const ColFwdParams& fp = *(const ColFwdParams*)(KFP*)__builtin_amdgcn_kernarg_segment_ptr();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int sh[2];   // 0: dequeued item, 1: last workgroup
  rr_ts(0, 7);
  rr_ts_edge(0);
  FusedSync* sy = fp_arg.sync;
  int* done = reinterpret_cast<int*>(sy + 1);
  const int nst = fp_arg.nst, nqs = fp_arg.nq, spin_limit = fp_arg.spin_limit;
  const int B = fp.st[0].a.B, U = fp.st[0].a.U, strips = fp.st[0].strips;
  const int ips = U * strips;   // items per (stage, slot) = a slot's dependency count
  const int q = xcc_id() % nqs;
  const int nbq = (B - q + nqs - 1) / nqs;
  const int per_stage = nbq * ips;
  const int total = nst * per_stage;
  int* head = &sy->head[q];
  const int wave = __builtin_amdgcn_readfirstlane(nrx_tid() >> 6);
  if (nrx_tid() == 0) {
    sh[0] = atomicAdd(head, 1);
    if (fp_arg.dbg_err && blockIdx.x == 0)
      __hip_atomic_fetch_or(&sy->err, fp_arg.dbg_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  int j = sh[0], k = 0;
  auto decode = [&](int jj, int s, int& b, int& u, int& strip) {
    const int r = jj - s * per_stage;
    b = q + nqs * (r / ips);
    const int ru = r % ips;
    u = ru / strips;
    strip = ru % strips;
  };
  // Fast path of the three-stage forward (num_it = 2, the bench shape): a workgroup whose
  // dequeues return one item of each stage in turn -- the case at most one item per CU and
  // stage gives -- runs them as straight-line code.  A loop around the item bodies kept their
  // thread-derived addresses live across every body (164 VGPRs of spills for the three kinds,
  // 16-25 for one); here each body sees only its own.  Any other dequeue falls through to the
  // generic loop below, so every item is run whatever the dequeue order.
  if (nst == 3 && j < per_stage) {
    int b, u, strip;
    decode(j, 0, b, u, strip);
    fwd_col_item<CHP, 0>(fp.st[0], smem, wave, b, u, strip, k++);
    j = fwd_col_done(done + b, head, sh);
    if (j >= per_stage && j < 2 * per_stage) {
      decode(j, 1, b, u, strip);
      fused_wait(done + b, ips, sy, spin_limit);
      NRX_FC_WAIT_STAMP(k);
      fwd_col_item<CHP, 1>(fp.st[1], smem, wave, b, u, strip, k++);
      j = fwd_col_done(done + B + b, head, sh);
      if (j >= 2 * per_stage && j < total) {
        decode(j, 2, b, u, strip);
        fused_wait(done + B + b, ips, sy, spin_limit);
        NRX_FC_WAIT_STAMP(k);
        fwd_col_item<CHP, 2>(fp.st[2], smem, wave, b, u, strip, k++);
        j = fwd_col_done(done + 2 * B + b, head, sh);
      }
    }
  }
  while (j < total) {
    const int s = j / per_stage;
    int b, u, strip;
    decode(j, s, b, u, strip);
    if (s >= 1) fused_wait(done + (s - 1) * B + b, ips, sy, spin_limit);
    NRX_FC_WAIT_STAMP(k);
    if (s == 0) fwd_col_item<CHP, 0>(fp.st[0], smem, wave, b, u, strip, k);
    else if (s < nst - 1) fwd_col_item<CHP, 1>(fp.st[s], smem, wave, b, u, strip, k);
    else fwd_col_item<CHP, 2>(fp.st[s], smem, wave, b, u, strip, k);
    j = fwd_col_done(done + s * B + b, head, sh);
    ++k;
  }
  rr_ts_edge(1);
  // the last workgroup to leave checks every counter and resets them for the next forward
  if (nrx_tid() == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    sh[1] = atomicAdd(&sy->exits, 1) == (int)(gridDim.x * gridDim.y) - 1;
  }
  __syncthreads();
  if (sh[1]) {
    for (int i = nrx_tid(); i < nst * B; i += 512)
      if (__hip_atomic_load(done + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ips)
        __hip_atomic_fetch_or(&sy->err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    for (int i = nrx_tid(); i < nst * B; i += 512) done[i] = 0;
    if (nrx_tid() < 8) sy->head[nrx_tid()] = 0;
    if (nrx_tid() == 0) sy->exits = 0;
  }
}
