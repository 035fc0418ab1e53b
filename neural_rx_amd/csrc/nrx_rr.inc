// nrx_rr.inc -- register-resident UpdateState launch (k_update_rr), f16, any U (for U > 2 conv1
// reads the a_u planes the combine pass wrote).  The default schedule runs the aggregation
// updates here and the readout update on the strip kernel (nrx_update_schedule, DESIGN.md 14).
//
// Same math, same HBM layout and bit-identical outputs to k_update's GZ items (UpdateState,
// copy_pytorch.py:267-287; AggregateUserStates / readouts fused into the conv3 epilogue,
// neural_rx.py:135-207, 309-404); a different schedule inside the workgroup (DESIGN.md
// sections 13-14):
//
// * Stage-resident weights.  One workgroup per CU loops over the stage's items; the three
//   separable layers' images and the aggregation MLP (107 KB) are staged into LDS once per
//   launch, not once per item.
// * Register-resident activations.  An item is one (slot, user, strip of 16 subcarriers); its
//   strip positions 1..20 (conv1 rows: 16 outputs + the 2-row halo each side) are OWNED by the
//   8 waves, R = 3 for waves 0-3 and 2 for waves 4-7 (waves w and w + 4 share a SIMD: 5 rows per
//   SIMD).  A layer's output stays in the owning wave's registers as the next layer's B
//   fragments: the MFMA C layout of tiles 2kc, 2kc+1 is chunk 4kc + g of the consumer (host
//   K-permutation, the same packing as the strip kernels' in-place image), so a transition
//   writes only each wave's first and last row to LDS (the neighbours' depthwise halo rows:
//   14 x 3.5 KB, laid out without bank conflicts: rr_exch_lo) instead of the whole 128-channel
//   strip.
// * conv1 reads its z rows [a | s | pe] straight from memory (GZ, struct GZ), as k_update's
//   GZ items do: no z image.
// * The symbol-axis padding lanes t = 14, 15 of conv1 / conv2 outputs must be zero (they are
//   the t+1 neighbour of t = 13 in the next depthwise): their C operand (the bias of the first
//   K chunk) is read from a block of -inf, so the column comes out -inf and the ReLU makes it 0.
//
// Every MFMA sees the operands of the strip kernel's in the same order (bias as the C operand of
// K chunk 0, chunks 0..3, the same depthwise), so the outputs equal k_update's bit for bit
// (tests/test_gpu_update_rr.py).  (Included inside namespace nrx by nrx_k_rr.hip.)

// A/B switch (variant libraries): out-of-grid rows zeroed behind a uniform branch instead of a
// select per register (+0.6 %, profiles/r05/ab_update_schedule.txt)
#ifndef NRX_RR_ZBRANCH
#define NRX_RR_ZBRANCH 1
#endif

// (the item geometry kRrFO .. and the LDS plan kRrW1 .. kRrLds, rr_heads_fit: nrx_geom.h)

// Diagnostic builds (NRX_STAMPS): s_memtime of lane 0 of waves 0 and 4 at the phase ends of the
// workgroup's items k < 4: g_nrx_rr_stamps[wg][16 k + 2 m + (wave == 4)], m = 0 item start,
// 1 conv1 math, 2 conv1 rows exchanged, 3 conv2 math, 4 conv2 rows exchanged, 5 conv3 math,
// 6 item done, and (k = 0, m = 7) the kernel start, before the weight staging (tools/stamps_rr.py).
#ifdef NRX_STAMPS
__device__ __forceinline__ void rr_ts(int k, int m) {
  if ((nrx_tid() & 255) == 0 && g_nrx_stamp_on && k < 4 && blockIdx.x < 4096)
    g_nrx_rr_stamps[blockIdx.x][16 * k + 2 * m + (nrx_tid() >> 8)] = __builtin_amdgcn_s_memtime();
}
// wave 0 of the workgroup: s_memrealtime (100 MHz) at the kernel start (e = 0, slot k = 1, m = 7) and
// end (e = 1, k = 2, m = 7) and s_memtime at the end (k = 3, m = 7): the wall span and the clock
__device__ __forceinline__ void rr_ts_edge(int e) {
  if (nrx_tid() == 0 && g_nrx_stamp_on && blockIdx.x < 4096) {
    g_nrx_rr_stamps[blockIdx.x][16 * (1 + e) + 14] = __builtin_amdgcn_s_memrealtime();
    if (e) g_nrx_rr_stamps[blockIdx.x][16 * 3 + 14] = __builtin_amdgcn_s_memtime();
  }
}
#else
__device__ __forceinline__ void rr_ts(int, int) {}
__device__ __forceinline__ void rr_ts_edge(int) {}
#endif

// first owned strip position of wave w: waves 0-3 own 3 rows (1-3, 4-6, 7-9, 10-12), 4-7 own 2
// (13-14, 15-16, 17-18, 19-20)
__device__ __forceinline__ int rr_r0(int w) { return w < 4 ? 1 + 3 * w : 13 + 2 * (w - 4); }
// exchange slot of wave w's first (side 0) / last (side 1) own row
__device__ __forceinline__ int rr_slot(int w, int side) { return 2 * w + side - 1; }

typedef const __attribute__((address_space(3))) char rr_lds_cchar;
typedef __attribute__((address_space(3))) char rr_lds_char;
typedef const __attribute__((address_space(3))) half8 rr_lds_chalf8;
typedef __attribute__((address_space(3))) half8 rr_lds_half8;
typedef const __attribute__((address_space(3))) floatx4 rr_lds_cfloatx4;
__device__ __forceinline__ unsigned rr_lds_addr(const char* p) { return (unsigned)(size_t)(rr_lds_cchar*)p; }

// A separable layer's LDS image with a per-lane bias row: conv1 / conv2 read the -inf block
// for the pad symbols.  The lane's bias address (+16 g) is one opaque register, so every
// tile's C operand is one ds_read_b128 with an immediate offset.
template <int COUTP>
struct WRr {
  WLds<P16, kHID, COUTP> w;
  unsigned boff;
  __device__ WRr(const char* base, const char* bias_row, int g) : w{base} {
    boff = rr_lds_addr(bias_row) + 16u * (unsigned)g;
    asm("" : "+v"(boff));
  }
  __device__ half8 afrag(int n, int kc, int lane, int g) const { return w.afrag(n, kc, lane, g); }
  __device__ void dw_taps(int kc, int g, half8 (&t)[9]) const { w.dw_taps(kc, g, t); }
  __device__ floatx4 bias_acc(int n, int) const { return *(rr_lds_cfloatx4*)((rr_lds_cchar*)(size_t)boff + 64 * n); }
};

// Exchange-row slot of lane (t < 14, g) in a K chunk's 896 B: the symbols of channel group g
// rotated by 2 g, and the zero-block slot the pad lanes (t = 14, 15) of group g read.  With
// these, every ds_read_b128 lane group ({0-3, 12-15, 20-27}, ..., MI355X_MICROARCH.md) hits 15
// distinct 16-byte bank quads (14 data slots + one zero slot) and every 8-lane ds_write_b128
// group 8 distinct quads: no bank conflicts (the plain (14 g + t) order put lanes of g = 0 and
// g = 1 on the same banks: 9.7 % of the launch's LDS cycles, profiles/r05/sq_rr_vs_strip).
__device__ __forceinline__ unsigned rr_exch_lo(int g, int t) {
  int s = t + 2 * g;
  s = s >= kT ? s - kT : s;
  return (unsigned)((g * kT + s) * 16);
}
__device__ __forceinline__ unsigned rr_zero_lo(int g) {   // quads 14, 12, 8, 10 (kRrX = kRrZero mod 256)
  return (unsigned)(16 * (g == 0 ? 14 : g == 1 ? 12 : g == 2 ? 8 : 10));
}
static_assert((kRrX - kRrZero) % 256 == 0 && 16 * 15 + 3 * kRrExChunk + 16 <= kRrX - kRrZero,
              "zero slots must share the exchange rows' bank phase and stay inside the zero block");

// Lane addresses of a wave's neighbour exchange rows (chunk 0; chunk kc at + kc * 896 as the DS
// immediate): lanes t >= 14 read the zero block.
struct RrNb {
  unsigned top, bot;
};
__device__ __forceinline__ RrNb rr_nb(const char* smem, int wave, int t, int g) {
  const unsigned zero = rr_lds_addr(smem + kRrZero) + rr_zero_lo(g);
  const unsigned lo = rr_exch_lo(g, t);
  RrNb nb;
  nb.top = (t < kT && wave > 0) ? rr_lds_addr(smem + kRrX + rr_slot(wave - 1, 1) * kRrExRow) + lo : zero;
  nb.bot = (t < kT && wave < 7) ? rr_lds_addr(smem + kRrX + rr_slot(wave + 1, 0) * kRrExRow) + lo : zero;
  asm("" : "+v"(nb.top), "+v"(nb.bot));
  return nb;
}
__device__ __forceinline__ half8 rr_ld(unsigned a, int kc) {
  return *(rr_lds_chalf8*)((rr_lds_cchar*)(size_t)a + kc * kRrExChunk);
}

// Output rows own[A .. B) of a wave (own-row indices; -1 = the row above own row 0, RO = the row
// below own row RO - 1, both from the exchange rows) x COUTP channels, bias included.  The
// taps and the neighbour rows of chunk kc + 1 are read once chunk kc's depthwise is done (as
// conv_rows); every A fragment is reused over the B - A rows.
template <int RO, int A, int B, int COUTP, class WS>
__device__ __forceinline__ void rr_pass(const half8 (&in)[RO][4], const RrNb& nb, const WS& ws, int lane, int g,
                                        floatx4 (&acc)[B - A][COUTP / 16]) {
  constexpr int NR = B - A;
  constexpr int NT = COUTP / 16;
  constexpr bool TOP = A == 0, BOT = B == RO;
  static_assert(NR >= 1 && A >= 0 && B <= RO, "rows");
  half8 w[9], xt{}, xb{};
  auto load = [&](int kc) {
    if constexpr (TOP) xt = rr_ld(nb.top, kc);
    if constexpr (BOT) xb = rr_ld(nb.bot, kc);
    ws.dw_taps(kc, g, w);
  };
  load(0);
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) {
    half8 a_cur = ws.afrag(0, kc, lane, g);
    half8 d[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = A + r;   // output own-row index; inputs i-1, i, i+1
      const half8 x0 = i - 1 < 0 ? xt : in[i - 1 < 0 ? 0 : i - 1][kc];
      const half8 x2 = i + 1 >= RO ? xb : in[i + 1 >= RO ? RO - 1 : i + 1][kc];
      d[r] = P16::dw_row(x0, in[i][kc], x2, w);
    }
    dw_fence<NR>(d);
    if (kc + 1 < 4) load(kc + 1);
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

// conv1 / conv2 accumulators of own rows [A, B) -> f16 B fragments (ReLU), rows outside the grid
// zero (SAME padding of the next depthwise).  The packing is EpiInPlace's: the lane's values of
// tiles 2kc, 2kc+1 are its chunk kc of the consumer.
template <int RO, int A, int B>
__device__ __forceinline__ void rr_to_own(const floatx4 (&acc)[B - A][8], half8 (&own)[RO][4], int f_own0, int F) {
#pragma unroll
  for (int r = 0; r < B - A; ++r) {
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const floatx4& a0 = acc[r][2 * kc];
      const floatx4& a1 = acc[r][2 * kc + 1];
      half8 h = half8{(_Float16)a0[0], (_Float16)a0[1], (_Float16)a0[2], (_Float16)a0[3],
                      (_Float16)a1[0], (_Float16)a1[1], (_Float16)a1[2], (_Float16)a1[3]};
      h = __builtin_elementwise_max(h, half8{});
      if constexpr (!NRX_RR_ZBRANCH) {
        const int f = f_own0 + A + r;
        if (f < 0 || f >= F) h = half8{};
      }
      own[A + r][kc] = h;
    }
  }
  if constexpr (!NRX_RR_ZBRANCH) return;
  // rows outside the grid exist only in a slot's first and last strips: a wave-uniform branch
  // around the zeroing instead of a select on every register of every row
  const int fa = f_own0 + A, fb = f_own0 + B - 1;
  if (__builtin_expect(fa < 0 || fb >= F, 0)) {
#pragma unroll
    for (int r = 0; r < B - A; ++r) {
      const int f = f_own0 + A + r;
      if (f < 0 || f >= F) {
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) own[A + r][kc] = half8{};
      }
    }
  }
}

// The wave's first and last own rows into its exchange slots (lanes t < 14).
template <int RO>
__device__ __forceinline__ void rr_write_exch(char* smem, int wave, int t, int g, const half8 (&own)[RO][4]) {
  if (t >= kT) return;
  const unsigned lo = rr_exch_lo(g, t);
  if (wave > 0) {
    const unsigned a = rr_lds_addr(smem + kRrX + rr_slot(wave, 0) * kRrExRow) + lo;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) *(rr_lds_half8*)((rr_lds_char*)(size_t)a + kc * kRrExChunk) = own[0][kc];
  }
  if (wave < 7) {
    const unsigned a = rr_lds_addr(smem + kRrX + rr_slot(wave, 1) * kRrExRow) + lo;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) *(rr_lds_half8*)((rr_lds_char*)(size_t)a + kc * kRrExChunk) = own[RO - 1][kc];
  }
}

// conv1 / conv2 of own rows [A, B) into own[] (a scope of their own: the accumulators die here)
template <int RO, int A, int B>
__device__ __forceinline__ void rr_layer_own(half8 (&own)[RO][4], const RrNb& nb, const WRr<kHID>& ws, int lane, int g,
                                             int f_own0, int F) {
  floatx4 acc[B - A][8];
  rr_pass<RO, A, B, kHID>(own, nb, ws, lane, g, acc);
  rr_to_own<RO, A, B>(acc, own, f_own0, F);
}

// conv3 of own rows [A, B) and the fused epilogue (new state + next aggregation MLP, or the
// readout heads), EpiConv3 as in the strip kernels: p0 = strip position of own row A.
template <int RO, int A, int B, class Epi>
__device__ __forceinline__ void rr_conv3(const half8 (&own)[RO][4], const RrNb& nb, Epi& epi, int lane, int t, int g,
                                         int p0, int kst = 0) {
  typename Epi::template PrefT<B - A> pf;
  epi.template prefetch<B - A>(pf, p0, t, g);   // skip-connection rows, in flight during the math
  floatx4 acc[B - A][4];
  rr_pass<RO, A, B, kDSP>(own, nb, epi.ws, lane, g, acc);
  rr_ts(kst, 5);
  epi.template settle<B - A>(pf);
  epi.template run<B - A>(acc, pf, p0, t, g, 0, B - A);
}

// Readout heads (TAIL_READOUT_WB layout) staged into the exchange region once every wave is
// past its conv3 reads; the global loads are issued before the conv3 math.
template <int CHP>
struct RrHeads {
  DenseStage<kDSP, kHID> l1, c1;
  DenseStage<kHID, 16> l2;
  DenseStage<kHID, CHP> c2;
  __device__ __forceinline__ void load(const BlockParams<P16>& prm) {
    l1.load(prm.llr[0][0]);
    l2.load(prm.llr[0][1]);
    c1.load(prm.chest[0]);
    c2.load(prm.chest[1]);
  }
  __device__ __forceinline__ void store(char* WB, const BlockParams<P16>& prm) const {
    const int nb2 = prm.a.bits_max;
    l1.store(WB, reinterpret_cast<float*>(WB + kHB1));
    c1.store(WB + kHW1C, reinterpret_cast<float*>(WB + kHB1 + kHID * 4));
    l2.store(WB + kHW2, reinterpret_cast<float*>(WB + kHB2), nb2);
    c2.store(WB + kHW2 + nb2 * 256, reinterpret_cast<float*>(WB + kHB2 + 16 * 4), 2 * prm.a.A);
  }
};

// Readout variant of rr_conv3: the heads go into X, which the conv3 math still reads, so every
// wave (also one with no conv3 rows, B == A) runs conv3, a barrier, its share of the head stores,
// a barrier, and only then the readout epilogue from the held accumulators.
template <int RO, int A, int B, class Epi, class Hd>
__device__ __forceinline__ void rr_conv3_ro(const half8 (&own)[RO][4], const RrNb& nb, Epi& epi, const Hd& hd,
                                            const BlockParams<P16>& prm, char* X, int lane, int t, int g, int p0,
                                            int kst = 0) {
  constexpr int NR = B - A;
  constexpr int NRA = NR > 0 ? NR : 1;
  typename Epi::template PrefT<NRA> pf;
  floatx4 acc[NRA][4];
  if constexpr (NR > 0) {
    epi.template prefetch<NR>(pf, p0, t, g);
    rr_pass<RO, A, B, kDSP>(own, nb, epi.ws, lane, g, acc);
  }
  rr_ts(kst, 5);
  __syncthreads();   // every wave is past its conv3 reads of X
  hd.store(X, prm);
  __syncthreads();
  if constexpr (NR > 0) {
    epi.template settle<NR>(pf);
    epi.template run<NR>(acc, pf, p0, t, g, 0, NR);
  }
}

// The wave's GZ addressing of item (b, u, strip) and its first K chunk of the RO + 2 input rows.
// (Issuing it one item ahead, during the previous epilogue, measured -0.5 %: the epilogue's own
// loads and stores queue behind it; under the weight staging it delayed the staging by 2.8 k
// cycles -- profiles/r05/stamps_rr_ahead.txt.)
template <int RO>
__device__ __forceinline__ void rr_gz_first(GZ& gz, const BlockParams<P16>& prm, int wave, int b, int u, int strip) {
  const int lane = nrx_tid() & 63, t = lane & 15, g = lane >> 4;
  const int r0 = rr_r0(wave);
  gz = gz_make(prm, b, u, strip * kRrFO - kHalo, t, g);
#pragma unroll
  for (int i = 0; i < RO + 2; ++i) gz.x0[i] = gz.load(0, gz.row_soff(r0 - 1 + i));
}

// One item (slot b, user u, strip) on the calling wave, which owns RO rows from position r0.
// Every wave runs the same barriers in the same order (RO = 3 and 2 bodies alike).
template <int RO, int CHP, int TAILM>
__device__ __forceinline__ void rr_item(const BlockParams<P16>& prm, char* smem, int wave, int b, int u, int strip,
                                        int k) {
  rr_ts(k, 0);
  constexpr bool RO3 = RO == 3;
  const int lane = nrx_tid() & 63, t = lane & 15, g = lane >> 4;
  const int r0 = rr_r0(wave);
  const int f_start = strip * kRrFO - kHalo;
  const int F = prm.a.F;
  const int f_own0 = f_start + r0;
  char* X = smem + kRrX;
  const RrNb nb = rr_nb(smem, wave, t, g);
  half8 own[RO][4];
  GZ gz;
  rr_gz_first<RO>(gz, prm, wave, b, u, strip);
  // ---- conv1: z rows [a | s | pe] from memory (GZ), every own row
  {
    const WRr<kHID> w1(smem + kRrW1, t < kT ? smem + kRrW1 + kWBias : smem + kRrNeg + kRrNegOff, g);
    floatx4 acc[RO][8];
    conv_rows<P16, kUPD_CINP, kHID, RO, WRr<kHID>, true, true>(nullptr, r0, kRrSlots, t, g, lane, w1, acc, &gz);
    rr_to_own<RO, 0, RO>(acc, own, f_own0, F);
  }
  rr_ts(k, 1);
  __syncthreads();   // every wave is past the previous item's reads of X (conv3 rows, heads)
  rr_write_exch<RO>(smem, wave, t, g, own);
  __syncthreads();
  rr_ts(k, 2);
  // ---- conv2 (positions 2..19): wave 0 skips own row 0 (position 1), wave 7 own row 1 (20)
  {
    const WRr<kHID> w2(smem + kRrW2, t < kT ? smem + kRrW2 + kWBias : smem + kRrNeg + kRrNegOff, g);
    if constexpr (RO3) {
      if (wave == 0) rr_layer_own<3, 1, 3>(own, nb, w2, lane, g, f_own0, F);
      else rr_layer_own<3, 0, 3>(own, nb, w2, lane, g, f_own0, F);
    } else {
      if (wave == 7) rr_layer_own<2, 0, 1>(own, nb, w2, lane, g, f_own0, F);
      else rr_layer_own<2, 0, 2>(own, nb, w2, lane, g, f_own0, F);
    }
  }
  rr_ts(k, 3);
  __syncthreads();   // every wave is past its conv2 reads of the conv1 exchange rows
  rr_write_exch<RO>(smem, wave, t, g, own);
  __syncthreads();
  rr_ts(k, 4);
  // ---- conv3 (positions 3..18) + the fused epilogue: wave 0 computes own row 2 only, wave 7 none
  using WS3 = WLds<P16, kHID, kDSP>;
  const WS3 w3{smem + kRrW3};
  char* WB = TAILM == TAIL_READOUT_WB ? X : smem + kRrW3;
  EpiConv3<P16, WS3, CHP, TAILM> epi{&prm, nullptr, WB, w3, b, u, f_start, kRrSlots - kHalo, 0, 1.f, false,
                                     (float)prm.a.active[(size_t)b * prm.a.U + u], -1, 0, 0};
  epi.pos_lo = kHalo;
  if constexpr (TAILM == TAIL_READOUT_WB) {
    RrHeads<CHP> hd;
    hd.load(prm);
    if constexpr (RO3) {
      if (wave == 0) rr_conv3_ro<3, 2, 3>(own, nb, epi, hd, prm, X, lane, t, g, r0 + 2, k);
      else rr_conv3_ro<3, 0, 3>(own, nb, epi, hd, prm, X, lane, t, g, r0, k);
    } else {
      if (wave == 7) rr_conv3_ro<2, 0, 0>(own, nb, epi, hd, prm, X, lane, t, g, r0, k);
      else rr_conv3_ro<2, 0, 2>(own, nb, epi, hd, prm, X, lane, t, g, r0, k);
    }
  } else {
    if constexpr (RO3) {
      if (wave == 0) rr_conv3<3, 2, 3>(own, nb, epi, lane, t, g, r0 + 2, k);
      else rr_conv3<3, 0, 3>(own, nb, epi, lane, t, g, r0, k);
    } else {
      if (wave != 7) rr_conv3<2, 0, 2>(own, nb, epi, lane, t, g, r0, k);
    }
  }
  rr_ts(k, 6);
}

// Stage the launch's weights into LDS once: the three layer images, the aggregation MLP (TAIL_AGG),
// the -inf and zero blocks.
// Every global load is issued before the first LDS store (~60 VGPRs, nothing else is live yet),
// so the staging waits for one round trip instead of one per image.
template <int TAILM>
__device__ __forceinline__ void rr_stage_weights(const BlockParams<P16>& prm, char* smem) {
  SepStage<kUPD_CINP, kHID> s1;
  SepStage<kHID, kHID> s2;
  SepStage<kHID, kDSP> s3;
  DenseStage<kDSP, kAGG> d1;
  DenseStage<kAGG, kDSP> d2;
  s1.load(prm.w[0]);
  s2.load(prm.w[1]);
  s3.load(prm.w[2]);
  if constexpr (TAILM == TAIL_AGG) {
    d1.load(prm.agg[0]);
    d2.load(prm.agg[1]);
  }
  s1.store(smem + kRrW1);
  s2.store(smem + kRrW2);
  s3.store(smem + kRrW3);
  if constexpr (TAILM == TAIL_AGG) {
    d1.store(smem + kRrW3 + 16 * 1024, reinterpret_cast<float*>(smem + kRrW3 + kWTailBias));
    d2.store(smem + kRrW3 + 24 * 1024, reinterpret_cast<float*>(smem + kRrW3 + kWTailBias + kAGG * 4));
  }
  for (int i = nrx_tid(); i < 768 / 4; i += 512) reinterpret_cast<float*>(smem + kRrNeg)[i] = -__builtin_inff();
  for (int i = nrx_tid(); i < kRrExChunk * 4 / 16; i += 512) reinterpret_cast<intx4*>(smem + kRrZero)[i] = intx4{0, 0, 0, 0};
}

// UpdateState of a whole stage: grid = min(items, CUs), one workgroup per CU (LDS), items
// i = blockIdx.x + k gridDim.x in work_item's XCD-grouped order (strips of 16 subcarriers).
template <int CHP, int TAILM>
__global__ __launch_bounds__(512) void k_update_rr(BlockParams<P16> prm, int items) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  rr_ts(0, 7);   // kernel start (diagnostic builds): the weight staging ends at item 0's start
  rr_ts_edge(0);
  const int wave = __builtin_amdgcn_readfirstlane(nrx_tid() >> 6);
  rr_stage_weights<TAILM>(prm, smem);
  __syncthreads();
  int k = 0;
  for (int i = blockIdx.x; i < items; i += gridDim.x, ++k) {
    int b, u, strip;
    work_item(i, prm.a.B, prm.a.U, prm.strips, prm.order_rev, b, u, strip);
    if (wave < 4) rr_item<3, CHP, TAILM>(prm, smem, wave, b, u, strip, k);
    else rr_item<2, CHP, TAILM>(prm, smem, wave, b, u, strip, k);
  }
  rr_ts_edge(1);
}
