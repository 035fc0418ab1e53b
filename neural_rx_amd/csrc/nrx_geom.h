// nrx_geom.h -- tile geometry and limits of the forward kernels (nrx_device.inc, nrx_rr.inc, nrx_col.inc) that the
// launch planner (plan_forward, nrx_dispatch.hip) reads too: constexpr values and functions only, no kernel.
#pragma once
#include "nrx_internal.h"

namespace nrx {

// TAIL_READOUT_WB: readout tail with the heads staged into WB, two items per workgroup
enum Tail { TAIL_NONE = -1, TAIL_AGG = 0, TAIL_READOUT = 1, TAIL_READOUT_WB = 2 };
constexpr bool readout_tail(int t) { return t == TAIL_READOUT || t == TAIL_READOUT_WB; }

constexpr unsigned kGzOob = kGzRange;              // > any workspace this path is taken for
// ---- the strip kernels (nrx_device.inc)
// Strip image in LDS: slot (one subcarrier row) x 16 symbols x up to 128 channels, with a
// fixed slot pitch so that every layer of a block can run in place in one buffer.
template <class P>
constexpr int slot_pitch() { return kTP * kHID * (int)sizeof(typename P::S); }

// Per-layer weight image in LDS (P16): layout constants kWPw .. kHW2 in nrx_internal.h
// (shared with the host, which packs the same images for the LDS-DMA of nrx_rr.inc).
// The paired readout tail gives WB the rest of the 160 KB LDS (P16: 160 KB - 30 x 4 KB) and
// stages the heads there, so that the strip image X is free for the next item's z DMA
// during the readout epilogue.  W1^T images in full; W2^T images truncated to their real
// rows (bits, 2A): the lanes of the padding rows read whatever follows, which only reaches
// output channels that are never stored.  One LLR head only.
constexpr int kWAlloc = 160 * 1024 - 30 * kTP * kHID * 2;
static_assert(kWBytes <= kWAlloc, "layer weight image exceeds the LDS left by the strip image");
// The truncated W2^T images put the LLR rows [0, bits_max) in the b2 slot of 16 outputs and
// the ChEst rows [0, 2A) in a CHP-row slot: bits_max <= 16 and 2A <= CHP <= 32 are
// required besides the byte budget (the padding rows the lanes read beyond the real ones
// only reach output channels that are never stored).
__host__ __device__ constexpr bool heads_fit_wb(int bits_max, int chp, int a2 = 0) {
  return bits_max <= 16 && a2 <= chp && chp <= 32 && kHW2 + 256 * (bits_max + chp) <= kWAlloc;
}

template <class P>
constexpr int strip_slots() { return P::FO + 2 * kHalo; }
template <class P>
constexpr int strip_lds_bytes(bool heads_wb = false) {
  return strip_slots<P>() * slot_pitch<P>() + (P::WLDS ? (heads_wb ? kWAlloc : kWBytes) : 0);
}
// Readout weight images staged into the (then free) strip buffer X (P16).
constexpr int kHeadSlot = 24 * 1024;   // W1^T 16 KB | W2^T <= 8 KB ... per head, 256-aligned
// slot grids above this many float4s get the separate k_norm pass (nrx_rt: 1 344)
constexpr int kNormFusedMaxQ = 8192;

// ---- k_forward (nrx_device.inc)
constexpr int kFusedMaxStages = 12;  // StateInit (x M for Var-IO) + the updates (8 for nrx_large);
                                     // FusedParams ~7.5 KB of kernel arguments (16 KB measured to
                                     // pass, tools/ubench/kernarg.hip)
// dynamic LDS of k_forward: the paired-readout layout minus room for the static __shared__
// words (the slot-norm reduction of StateInit, the queue words); the readout heads must fit
constexpr int kFusedLds = 160 * 1024 - 256;
// dynamic LDS of k_forward per strip tier: the 24-row tier's paired-readout layout fills the
// LDS, so it gives up 256 bytes of WB; the small-grid tiers (8 / 16-row strips) fit whole
template <class P>
constexpr int fused_lds() {
  return strip_lds_bytes<P>(true) > kFusedLds ? kFusedLds : strip_lds_bytes<P>(true);
}
constexpr int kFusedMaxB = 65536;
// logical stages: the StateInit stages, then per iteration (U > kInlineUsers) a combine stage
// and the update stage; one dependency counter row each
constexpr int kFusedMaxLS = 20;
constexpr int kFusedMaxUsers = 8;

// ---- the register-resident update launch (nrx_rr.inc)
constexpr int kRrFO = 16;                       // output subcarriers per item
constexpr int kRrSlots = kRrFO + 2 * kHalo;     // strip positions 0..21 (f = 16 strip - 3 + p)
constexpr int kRrExRow = 4 * kT * 4 * 16;       // one exchange row: 4 chunks x 14 symbols x 4 groups x 16 B
constexpr int kRrExChunk = kT * 4 * 16;         // 896 B per K chunk
constexpr int kRrExRows = 14;                   // first / last row of each wave but wave 0's first, wave 7's last
// LDS plan (dynamic, bytes): the three layer images (pw^T | taps | bias, WLds layout; conv3's
// image carries the aggregation MLP at +16 KB / +24 KB and its biases at kWTailBias, the strip
// kernels' WB layout, so EpiConv3 reads it unchanged), a block of -inf (conv1 / conv2 bias of the
// pad lanes), a zero block the pad lanes read as exchange rows, the exchange rows (which the
// readout launch reuses for its heads after conv3).
constexpr int kRrW1 = 0;
constexpr int kRrW2 = kRrW1 + kWTailBias;       // 35 584 B per 128-output image
constexpr int kRrW3 = kRrW2 + kWTailBias;
constexpr int kRrNeg = kRrW3 + kWBytes;         // conv3 + MLP image: 36 096 B
// the pad lanes' bias row starts kRrNegOff into a 768-byte block of -inf: the layers' bias rows
// sit at a multiple of 256 B, so the same offset would put a bias read and a -inf read of one
// ds_read_b128 lane group on the same banks
constexpr int kRrNegOff = 128;
constexpr int kRrZero = kRrNeg + 768;
constexpr int kRrX = kRrZero + kRrExChunk * 4;  // the pad lanes read zeros at every chunk offset
constexpr int kRrLds = kRrX + kRrExRows * kRrExRow;
static_assert(kRrLds <= 160 * 1024, "RR LDS plan exceeds the CU's LDS");
// the readout heads (TAIL_READOUT_WB layout) are staged into the exchange region after conv3
__host__ __device__ constexpr bool rr_heads_fit(int bits_max, int chp, int a2) {
  return bits_max <= 16 && a2 <= chp && chp <= 32 && kHW2 + 256 * (bits_max + chp) <= kRrExRows * kRrExRow;
}

// ---- the whole-column launches (nrx_col.inc)
constexpr int kColRO = 6;                  // own rows per wave
constexpr int kColPos = 8 * kColRO;        // positions per item
constexpr int kColFO = kColPos - 4;        // outputs per strip of a grid wider than kColPos
constexpr int kColRed = kRrLds;            // 8 doubles: slot_norm's wave partials
constexpr int kColLds = kColRed + 64;
static_assert(kColLds <= 160 * 1024, "column LDS plan exceeds the CU's LDS");
__host__ __device__ constexpr int col_strips(int F) { return F <= kColPos ? 1 : (F + kColFO - 1) / kColFO; }
constexpr int kColMaxStages = 1 + kMaxIt;
// Variants of the one-item column kernels (StagePlan::variant, set by plan_forward alone).  A lean variant takes as
// compile-time constants what is uniform over the launch and fixed by the bench family: one strip (no halo: every
// position 0 .. 47 is an output row of subcarrier f = position), the slot norm fused into StateInit, a model that
// takes h_hat, one StateInit (masking or one MCS), one LLR head of bits_max = 4, 2A = 8; the readout with or without the
// ChEst store (h_ref).  COL_GENERIC reads all of them from BlockParams at run time.
enum ColVariant { COL_GENERIC = 0, COL_LEAN = 1, COL_LEAN_NO_HREF = 2 };
struct ColGeneric {
  static constexpr bool kLean = false, kHref = true;
};
template <bool HREF>
struct ColLean {
  static constexpr bool kLean = true, kHref = HREF;
  static constexpr int kBits = 4, kA2 = 8;
};
#ifndef NRX_COL_LEAN
#define NRX_COL_LEAN 1   // 0: the plan never picks a lean variant (A/B switch)
#endif

}  // namespace nrx
