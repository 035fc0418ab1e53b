// nrx_internal.h -- shared between the HIP kernels and the host side of libnrx.so.
//
// Device data layout (see DESIGN.md "Data layout in HBM"):
//   state / aggregate buffers  s, a : [B][U][F][14][56]   (compact, no padding in HBM;
//                                     the kernels pad T -> 16 and channels in LDS)
//   storage type: _Float16 (NRX_PREC_F16) or float (NRX_PREC_F32X)
// Packed weights (one blob per precision, built by nrx_create: nrx_model.cpp):
//   separable conv: dw [9][CINP] (tap = i*3 + j, i along F, j along T),
//                   pwT [COUTP][CINP] (transposed pointwise kernel), bias [COUTP]
//   dense:          wT [COUTP][CINP], bias [COUTP]
//   WT = _Float16 / double, BT = float / double.  Zero padding everywhere.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/nrx.h"

namespace nrx {

constexpr int kT = 14;        // OFDM symbols (fixed by 5G NR slot)
constexpr int kTP = 16;       // padded symbol axis = MFMA tile width
constexpr int kDS = 56;       // state width d_s
constexpr int kDSP = 64;      // padded state width
constexpr int kHID = 128;     // conv hidden width / readout hidden width
constexpr int kAGG = 64;      // aggregation hidden width
constexpr int kUPD_CINP = 128;  // [a, s, pe] = 114 -> 128
constexpr int kMaxInit = 8;
constexpr int kMaxIt = 8;
// users whose leave-one-out combine the update z-load forms itself (the other user's act*sp plane
// IS a_u for U = 2); U >= 3 runs the f32 combine pass (k_combine / combine stages) and every
// update reads its a_u plane -- one rounding for every U > 2 and every schedule, and conv1 can
// read a_u from memory (GZ) for any U
constexpr int kInlineUsers = 2;
constexpr int kMaxHeads = 8;
constexpr int kMaxUsers = 16;
constexpr int kHalo = 3;      // 3 stacked 3x3 convs per block
// f16 workspaces stay below this many bytes: conv1's z-row loader (struct GZ) addresses the
// workspace through one buffer descriptor with 32-bit offsets and marks zero chunks with offsets
// at or beyond it; a larger forward runs in slot chunks (nrx_api.cpp chunk_slots)
constexpr unsigned kGzRange = 0x40000000u;
// StateInit pads each antenna block of its input z = [y | h | pe] to A2P channels; the weight packer
// (nrx_model.cpp) and the launchers (nrx_launch.inc) pick the kernels' A2P with this one rule
constexpr int init_a2p(int num_rx_ant) { return 2 * num_rx_ant <= 8 ? 8 : (2 * num_rx_ant <= 16 ? 16 : 32); }

// ---- workspaces (host).  Every block of a workspace starts on a 256-byte boundary of it.
inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
// The carver lays a workspace out: take() hands out the next block.  A null base is the size query: every
// block is null and bytes() the workspace size, so the size a caller is told and the pointers the kernels get
// come from one walk.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* ws) : base((char*)ws) {}
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align256(count * sizeof(T));
    return p;
  }
  size_t bytes() const { return off; }
};

// ---- LDS images of the f16 weights (kernels: SepStage / DenseStage).  A W^T [COUTP][CINP] image is a stack
// of 16-row tiles addressed like an activation image: element (co, chunk q of 8 inputs) at
// lds_off<NQ>(co >> 4, co & 15, q), NQ = CINP / 8 chunks per row, chunk index XOR-swizzled
// with the row so that a ds_read_b128 lane group hits distinct bank slots.
constexpr int kTPImg = 16;
__host__ __device__ constexpr int swz_q(int nq, int t) {
  return nq >= 16 ? (t & 15) : (nq == 8 ? ((t >> 1) & 7) : (nq == 4 ? ((t >> 2) & 3) : 0));
}
__host__ __device__ constexpr int lds_img_off(int nq, int row, int t, int q) {
  return ((row * kTPImg + t) * nq + (q ^ swz_q(nq, t))) * 16;
}
// separable layer: pw^T at 0 (<= 32 KB), dw [9][CINP] at kWPw, bias [COUTP] f32 at kWBias
constexpr int kWPw = kHID * kHID * 2;          // 32 KB
constexpr int kWDw = 9 * kHID * 2;             // 2304 B
constexpr int kWBias = kWPw + kWDw;            // conv bias [COUTP] f32
constexpr int kWTailBias = kWBias + kHID * 4;  // aggregation-MLP biases (2 x 64 f32)
constexpr int kWBytes = kWTailBias + 2 * kAGG * 4;
// readout heads (TAIL_READOUT_WB layout): LLR W1^T at 0, ChEst W1^T at kHW1C, biases, then
// the W2^T images truncated to their real rows
constexpr int kHW1C = 16 * 1024;                 // ChEst W1^T (LLR W1^T at 0)
constexpr int kHB1 = 32 * 1024;                  // b1: LLR [128] f32, ChEst [128] f32
constexpr int kHB2 = kHB1 + 2 * kHID * 4;        // b2: LLR [16] f32, ChEst [<= 32] f32
constexpr int kHW2 = kHB2 + (16 + 32) * 4;       // LLR W2^T rows [bits], then ChEst rows [2A]

template <class WT, class BT>
struct SepW {
  const WT* dw;
  const WT* pw;   // transposed [COUTP][CINP]
  const BT* b;
};

template <class WT, class BT>
struct DenseW {
  const WT* w;    // transposed [COUTP][CINP]
  const BT* b;
};

template <class WT, class BT>
struct ModelW {
  SepW<WT, BT> init[kMaxInit][3];
  DenseW<WT, BT> agg[kMaxIt][2];
  SepW<WT, BT> upd[kMaxIt][3];
  DenseW<WT, BT> llr[kMaxHeads][2];
  DenseW<WT, BT> chest[2];
};

// Shapes + pointers of one forward (kernel argument).
template <class WT, class BT, class S>
struct FwdArgs {
  int B, U, F, A, M, H;            // H = number of LLR heads
  int llr_B;                       // slots of the caller's llr tensor (the head stride; > B when
                                   // the forward runs in slot chunks, nrx_api.cpp)
  int init_cinp;                   // padded StateInit input width
  int num_init;
  int masking;
  int use_h;
  int bits_max;
  int head_bits[kMaxHeads];
  const float* y;                  // [B][F][T][2A]
  const float* pe;                 // [U][F][T][2]
  const float* h_hat;              // [B][U][F][T][2A] or null
  const float* active;             // [B][U]
  const float* mcs_mask;           // [B][U][M] or null
  float* llr;                      // [H][B][U][F][T][bits_max]
  float* h_ref;                    // [B][U][F][T][2A] or null
  double* norm;                    // [B] workspace
  S* s_in;                         // [B][U][F][14][56]
  S* s_out;
  S* a;                            // aggregate read by this update
  S* a_out;                        // aggregate written by the tail
  // one-launch forward (f16): the workspace as one buffer resource for conv1's z rows, and
  // the pe16 plane [U][F][14][56] (pe as f16 in channels 0, 1 of each 8-channel chunk 0;
  // written by the StateInit items, read as z chunk 14 by the update items' conv1)
  const char* ws_base;
  unsigned ws_bytes;
  S* pe16;
};

// The one-launch forward's control block (nrx_api.cpp fills it from the handle): the
// work-queue / counter buffer, the dependency-wait bound and debug error bits (nrx_debug_fused).
struct FusedCtl {
  void* sync;
  int spin_limit;
  int dbg_err;
};
// What the handle lets the planner choose from (plan_forward)
struct Sched {
  int mask;    // stage mask of the f16 forward (nrx_update_schedule; NRX_UPDATE_RR at nrx_create), bits below
  int fused;   // one-launch forwards (nrx_fused_config; NRX_FUSED): 0 off, 1 where measured faster, 2 where applicable
  int small = 1;   // the 8 / 16-row strip tiers for grids that leave CUs idle (tests switch them off to run the
                   // 24-row tier's kernels on a few slots: nrx_debug_small_tiers)
};
// schedule-mask bits of the three-launch f16 forward (nrx_update_schedule)
constexpr int kSchedRrAgg = 1, kSchedRrRo = 2, kSchedColAgg = 4, kSchedColRo = 8, kSchedColInit = 16;
constexpr int kSchedColFwd = 32;   // the one-launch column forward (k_fwd_col) where it applies
// bits 2 / 3 on grids wider than one 48-position column too (44-output strips with a halo; by
// default those grids keep the RR / strip updates, measured faster there: profiles/r06/configs)
constexpr int kSchedColWide = 64;
constexpr int kSchedMax = 127;
// default: the whole-column launches for every stage they apply to, the RR aggregation update
// where they do not (same-box A/B in profiles/r06/)
constexpr int kSchedDefault = kSchedColInit | kSchedColAgg | kSchedColRo | kSchedRrAgg;
constexpr int kFusedSpinLimit = 1 << 21;   // ~0.5 s of s_sleep 4 polls

// Optional per-kernel timing (nrx_profile_enable): events recorded around each launch on
// the launch stream.  Kernel ids:
enum KernelId {
  K_NORM = 0, K_INIT = 1, K_UPDATE = 2, K_FUSED = 3, K_UPDATE_RR = 4, K_COMBINE = 5, K_UPDATE_COL = 6, K_INIT_COL = 7,
  K_FWD_COL = 8, K_COUNT = 9
};

struct Prof {
  virtual void begin(int kid, void* stream) = 0;
  virtual void end(int kid, void* stream) = 0;
  virtual ~Prof() {}
};

// ---- the launch plan of one forward: which kernel runs each stage, on what grid.  plan_forward
// (nrx_dispatch.hip) alone decides it; the launchers (nrx_launch.inc, nrx_k_rr.hip, nrx_k_col.hip) execute it.
enum FwdPath { PATH_P16S, PATH_P16M, PATH_P16, PATH_FWD_COL, PATH_KFWD0, PATH_KFWD1, PATH_KFWD2, PATH_P64 };
enum StageKind { STAGE_STRIP, STAGE_RR, STAGE_COL };
struct StagePlan {       // stage s: StateInit m = s < num_init, else update i = s - num_init
  int kind;              // StageKind: the launcher
  int kid;               // KernelId the profiler charges the stage to
  int tail;              // the kernel variant's Tail ...
  int chp;               // ... its A2P (StateInit: 8 / 16 / 32) or CHP (update: 16 / 32) ...
  int one;               // ... the one-item column kernel (items <= grid), else the looping one
  int pair;              // ... strip update: two items per workgroup
  int items, strips;     // work items of the stage = B * U * strips
  int grid, lds;         // workgroups and dynamic LDS bytes of its launch (one-launch paths: FwdPlan's)
  int order_rev;         // BlockParams::order_rev: alternates with the launches
  int variant;           // ColVariant of a one-item column launch (nrx_geom.h): generic, or lean (with / without h_ref)
};
struct FwdPlan {
  int path;              // FwdPath
  int num_init, num_it;
  // launch-wide: the k_norm pre-pass runs; conv1 of the updates reads z from memory (GZ); the updates form the
  // leave-one-out combine themselves (U <= kInlineUsers), else k_combine launches / stages run
  int norm_pre, gz, inline_combine;
  int grid, lds, a2p, heads_x, nq;   // the one launch of k_fwd_col / k_forward (a2p: StateInit's; nq: queues)
  StagePlan st[kMaxInit + kMaxIt];
  bool one_launch() const { return path >= PATH_FWD_COL && path <= PATH_KFWD2; }
  bool combine_launches() const { return !inline_combine && !one_launch(); }
};
FwdPlan plan_forward(const FwdArgs<_Float16, float, _Float16>& a, int num_it, const Sched& sc, int cus, int xccs);
FwdPlan plan_forward(const FwdArgs<double, double, float>& a, int num_it);

// Aerial front/back-end (nrx_aerial.hip)
hipError_t launch_aerial_tables(const int32_t* ofdm_pos, const int32_t* sc_pos, int U, int nsym, int npil, int T,
                                int F, int32_t* nn, float* pe, hipStream_t st);
hipError_t launch_aerial_inputs(const float* y_re, const float* y_im, const float* h_re, const float* h_im,
                                const int32_t* nn, int B, int U, int F, int T, int A, int nsym, int npil, float* y,
                                float* h, hipStream_t st);
hipError_t launch_y_layout(const float* y0, const float* y1, int layout, int B, int F, int T, int A, float* y,
                           hipStream_t st);
hipError_t launch_aerial_llr(const float* llr, int B, int U, int F, int T, int bits_max, int bits, float* out,
                             hipStream_t st);

// Slot generator + error counters (nrx_synth.hip); struct types from include/nrx.h.
// elements of one [B][U][F][14] grid: x and the x' of the stages, complex f64
inline size_t gen_grid_elems(const nrx_gen_desc& d) {
  return (size_t)d.batch * d.num_tx * d.num_subcarriers * kT;
}
// the resolved carrier frequency offset of a generator call (nrx_cfo.hip)
struct GenCfo {
  double eps_max[16];                // cfo_hz[u] / subcarrier_spacing
  int constant;
  int fft_size;                      // N, resolved (never 0)
  int h_with_phase;
  double* eps_out;
};
// One generator call: what the checks of nrx_api.cpp (plan_gen) resolved, the optional stages (null: absent)
// and the blocks of its workspace.  gen_layout (nrx_synth.hip) alone knows their order.
struct GenPlan {
  nrx_gen_desc d;
  nrx_gen_chan c;                    // the resolved ports
  GenCfo cfo;
  bool cfo_on;                       // a port has a non-zero offset
  const nrx_gen_dmrs* dmrs;
  const nrx_gen_cir* cir;
  const nrx_gen_td* td;
  const nrx_gen_tc* tc;
  const double* no_slot;             // device [B] noise variance per slot (nrx_generate_slots_no), or null: d.no
  // byte offsets: behind the generator's own block at 0 the block of the one sample-domain stage (the x' of a
  // cfo, the x' and samples of a td, the buffers of a tc), the pilot table and the replayed channel
  size_t stage, pilots, cir_ws, total;
};
void gen_layout(GenPlan& p);
hipError_t launch_generate(const GenPlan& p, const nrx_gen_out& o, void* ws, hipStream_t st);
// the generator's own block: gen_workspace_bytes(d, nullptr, nullptr) = its size
struct GenWs;
size_t gen_workspace_bytes(const nrx_gen_desc& d, GenWs* w, void* base);
size_t dmrs_workspace_bytes(const nrx_gen_desc& d);
// nrx_generate_taps: the finished taps and delays of the built-in channel, rounded to f32
hipError_t launch_export_taps(const nrx_gen_desc& d, const nrx_gen_chan& c, float* a_out, float* tau_out, void* ws,
                              hipStream_t st);

// Channel impulse response replay (nrx_cir.hip); cir validated by nrx_generate_slots_cir.  x: [B][U][F][14]
// complex f64, the grid the channel acts on; ws: cir_workspace_bytes of the caller's workspace
size_t cir_workspace_bytes(const nrx_gen_desc& d);
hipError_t launch_cir_rx(const nrx_gen_desc& d, const nrx_gen_cir& c, const double* x, void* ws,
                         const double* no_slot, float* y, float* h, float* y_re, float* y_im, hipStream_t st);

// Despreading LS estimator (nrx_ls.hip); io validated by nrx_ls_estimate / nrx_generate_slots_dmrs
hipError_t launch_ls_estimate(const nrx_ls_io& io, hipStream_t st);
hipError_t launch_count_errors(const nrx_count_io& c, hipStream_t st);

// Carrier frequency offset (nrx_cfo.hip); validated by nrx_generate_slots_cfo / nrx_cfo_estimate /
// nrx_cfo_rotate.  x, xp: [B][U][F][14] complex f64 (re, im)
size_t cfo_workspace_bytes(const nrx_gen_desc& d);
hipError_t launch_cfo_apply(const nrx_gen_desc& d, const GenCfo& c, const double* x, const float* active, double* xp,
                            hipStream_t st);
hipError_t launch_cfo_h_phase(const nrx_gen_desc& d, const GenCfo& c, float* h, hipStream_t st);
hipError_t launch_cfo_estimate(const nrx_cfo_io& io, hipStream_t st);
hipError_t launch_cfo_rotate(const nrx_cfo_io& io, hipStream_t st);

// OFDM modulation / demodulation and the generator's time-domain stage (nrx_ofdm.hip); io validated by
// nrx_ofdm_modulate / nrx_ofdm_demodulate, td by nrx_generate_slots_td.  launch_td_apply: x [B][U][F][14]
// complex f64 -> x' at the start of ws (td_workspace_bytes), the samples behind it
hipError_t launch_ofdm(const nrx_ofdm_io& io, bool modulate, hipStream_t st);
// samples of one row: the symbols with their prefixes
inline int64_t slot_samples(const int32_t* cp_length, int fft_size, int num_symbols) {
  int64_t n = 0;
  for (int t = 0; t < num_symbols; ++t) n += cp_length[t] + fft_size;
  return n;
}
// the f64 planar nrx_ofdm_io of a generator stage s (nrx_gen_td, nrx_gen_tc) over `streams` rows per slot;
// the caller adds what only its stage has (amplifier, offsets, timing advance)
template <class Stage>
nrx_ofdm_io stage_ofdm(const nrx_gen_desc& d, const Stage& s, int streams, void* grid, void* samples) {
  nrx_ofdm_io io{};
  io.batch = d.batch, io.num_streams = streams, io.grid_subcarriers = d.num_subcarriers, io.num_symbols = kT;
  io.fft_size = s.fft_size, io.first_bin = s.first_bin;
  for (int t = 0; t < kT; ++t) io.cp_length[t] = s.cp_length[t];
  io.precision = NRX_OFDM_F64, io.grid_layout = NRX_OFDM_GRID_PLANAR;
  io.num_samples = slot_samples(s.cp_length, s.fft_size, kT);
  io.grid = grid, io.samples = samples;
  return io;
}
size_t td_workspace_bytes(const nrx_gen_desc& d, const nrx_gen_td& td);
hipError_t launch_td_apply(const nrx_gen_desc& d, const nrx_gen_td& td, const double* x, void* ws, hipStream_t st);
hipError_t launch_td_h_phase(const nrx_gen_desc& d, const nrx_gen_td& td, float* h, hipStream_t st);

// The time-domain channel and the generator's receive path through it (nrx_timechan.hip); io validated by
// nrx_time_channel, tc by nrx_generate_slots_tc.  tc_resolve_l_max: l_max, or for l_max < 0 the ceiling of the
// longest port delay in samples + 6.  launch_tc_taps: the sinusoid draws into ws (tc_workspace_bytes) and the
// window means of the taps into gt [B][U][A][L][14] (the generator's tap layout, so its antenna mixing applies);
// launch_tc_rx: modulate(x) -> channel -> demodulate -> y (+ the grid noise), h from the mean taps, r_out / x_out
hipError_t launch_time_channel(const nrx_tc_io& io, hipStream_t st);
int tc_resolve_l_max(const nrx_gen_desc& d, const nrx_gen_chan& c, const nrx_gen_tc& tc);
size_t tc_workspace_bytes(const nrx_gen_desc& d, const nrx_gen_tc& tc);
hipError_t launch_tc_taps(const nrx_gen_desc& d, const nrx_gen_chan& c, const nrx_gen_tc& tc, const double* tau,
                          const double* spdp, double* gt, void* ws, hipStream_t st);
hipError_t launch_tc_rx(const nrx_gen_desc& d, const nrx_gen_chan& c, const nrx_gen_tc& tc, const double* x,
                        const double* tau, const double* gt, void* ws, const double* no_slot, float* y, float* h,
                        float* y_re, float* y_im, hipStream_t st);

// LMMSE + max-log baseline detector (nrx_lmmse.hip); io validated by nrx_lmmse_detect
hipError_t launch_lmmse(const nrx_lmmse_io& io, hipStream_t st);

// K-best detector (nrx_kbest.hip); io validated by the nrx_kbest_* entry points
size_t kbest_workspace_bytes(const nrx_kbest_io& io);
hipError_t launch_kbest(const nrx_kbest_io& io, void* ws, hipStream_t st);

// Channel-estimation baselines (nrx_chest.hip); io validated by the nrx_cov_* / nrx_chest_* entry points
size_t cov_workspace_bytes(const nrx_cov_io& io);
hipError_t launch_cov_accumulate(const nrx_cov_io& io, void* ws, hipStream_t st);
size_t cov_space_workspace_bytes(const nrx_cov_space_io& io);
hipError_t launch_cov_space(const nrx_cov_space_io& io, void* ws, hipStream_t st);
hipError_t launch_chest_lmmse(const nrx_chest_io& io, hipStream_t st);
hipError_t launch_chest_lin(const nrx_chest_io& io, hipStream_t st);
size_t chest3_workspace_bytes(const nrx_chest3_io& io);
hipError_t launch_chest_lmmse3(const nrx_chest3_io& io, void* ws, hipStream_t st);

// Soft-output metrics (nrx_softmetrics.hip); io validated by the nrx_llr_stats* / nrx_nmse* entry points
constexpr int kSoftFS = NRX_SOFT_STRIP;   // subcarriers per work item
size_t llr_stats_workspace_bytes(const nrx_llr_stats_io& io);
hipError_t launch_llr_stats(const nrx_llr_stats_io& io, void* ws, hipStream_t st);
size_t nmse_workspace_bytes(const nrx_nmse_io& io);
hipError_t launch_chest_nmse(const nrx_nmse_io& io, void* ws, hipStream_t st);

// QC-LDPC decoder and slot glue (nrx_ldpc.hip); io validated by the nrx_ldpc_* entry points
struct LdpcPlan {
  int G;                             // codewords per workgroup
  int threads;
  int lds_bytes;                     // dynamic LDS: APP, and the messages when msg_lds
  bool msg_lds;                      // else the messages live in the workspace, [num_cw][num_edges][z] f32
};
struct LdpcDev {
  int mb, nb, z, kb, num_edges;
  LdpcPlan plan;
  const int* row_ptr;                // device [mb + 1]
  const int* edges;                  // device [num_edges][2]: (base column * z, shift)
};
LdpcPlan ldpc_plan(int nb, int z, int num_edges);
hipError_t ldpc_setup();
hipError_t launch_ldpc_decode(const LdpcDev& d, const nrx_ldpc_io& io, void* ws, hipStream_t st);
hipError_t launch_ldpc_gather(const nrx_ldpc_gather_io& io, hipStream_t st);
hipError_t launch_ldpc_count(const nrx_ldpc_count_io& io, hipStream_t st);

// Training (nrx_train.hip); desc and io validated by the nrx_train_* / nrx_adam_step entry points.  c1, c2: the
// bias corrections 1 - beta^step
size_t train_workspace_bytes(const nrx_desc& d, const nrx_train_io& io);
// accumulate: grad and loss are added onto, not overwritten; batch_total: the B of every loss denominator
hipError_t launch_train_grad(const nrx_desc& d, const nrx_train_io& io, bool accumulate, int batch_total, void* ws,
                             hipStream_t st);
hipError_t launch_adam(const nrx_adam_io& io, double c1, double c2, hipStream_t st);

hipError_t launch_llr_demap(const float* llr, int B, int U, int F, int T, int bits_stride, int bits,
                            const int32_t* data_re, int n_data, float* out, hipStream_t st);

}  // namespace nrx
