/*
 * nrx.h -- C ABI of the MI355X CGNN neural-receiver engine (libnrx.so).
 *
 * Plain C, plain pointers and sizes: no torch, no HIP types in the signatures
 * (streams are passed as `void*` = hipStream_t).  Every entry point returns an int
 * status (NRX_OK = 0, negative on error) and never throws; the last error message of
 * the calling thread is available from nrx_last_error().
 *
 * The reference has no FFI for this path: its hot path is a Python layer call,
 *   CGNN.forward([y, pe, h_hat, active_tx, mcs_ue_mask]) -> (llrs, h_hats)
 *       (utils/neural_rx.py:544-595; faithful TF structure in
 *        utils/neural_rx copy_pytorch.py:474-514),
 * wrapped by CGNNOFDM.forward (neural_rx.py:813-881) and
 * NeuralReceiverONNX.forward (neural_rx.py:1773-1812).  The entry points below are
 * what a binding of that call needs; INTEGRATION.md shows the
 * ctypes binding the Python layer uses.
 *
 * Layouts (all channels-last, as the reference's NHWC tensors):
 *   y        [B][F][T][2A]          f32  channels [Re a0..a(A-1), Im a0..a(A-1)]
 *   pe       [U][F][T][2]           f32  [time, freq] nearest-pilot encoding
 *   h_hat    [B][U][F][T][2A]       f32  initial channel estimate (NULL if unused)
 *   active   [B][U]                 f32  1 = DMRS port active
 *   mcs_mask [B][U][M]              f32  Var-IO state-init mixing weights (NULL: one-hot m=0)
 *   llr      [H][B][U][F][T][bits_max] f32 out, H = number of LLR heads
 *                                   (M for Var-IO, 1 otherwise); head h fills its
 *                                   first bits_h entries, the rest are written 0
 *   h_ref    [B][U][F][T][2A]       f32 out (NULL to skip the ChEst readout)
 * Sign convention: Sionna's LLR = log p(b=1)/p(b=0) (the Aerial layout negates,
 * neural_rx.py:1811; the Python layer does that, not the kernels).
 *
 * Besides the CGNN, the library holds what an evaluation loop needs on the device: the seeded
 * slot generator and the uncoded error counters, and the classical baseline detector the
 * reference's tables put next to the NRX (per-RE MIMO LMMSE + max-log demapper;
 * utils/baseline_rx.py), which reads the generator's tensors and writes LLRs in the layout above.
 */
#ifndef NRX_H_
#define NRX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRX_API_VERSION 7

enum nrx_status {
  NRX_OK = 0,
  NRX_ERR_INVALID_ARG = -1,   /* null pointer / bad enum / bad num_it */
  NRX_ERR_SHAPE = -2,         /* shape inconsistent with the model or limits */
  NRX_ERR_UNSUPPORTED = -3,   /* topology the kernels are not built for */
  NRX_ERR_HIP = -4,           /* HIP runtime error (message has the HIP string) */
  NRX_ERR_NOMEM = -5,
  NRX_ERR_WORKSPACE = -6,     /* workspace too small */
  NRX_ERR_BUSY = -7,          /* a forward of this handle is still running on another stream */
  NRX_ERR_FUSED = -8          /* an earlier one-launch forward reported an error: its outputs
                               * are invalid (see nrx_fused_status) */
};

/* Arithmetic of a forward pass. */
enum nrx_precision {
  NRX_PREC_F16 = 0,    /* perf mode: f16 activations, f16 depthwise, f16 MFMA with f32
                          accumulation (the reference's own TRT export ran --fp16) */
  NRX_PREC_F32X = 1    /* parity mode: f32 activations, f64 arithmetic (f64 MFMA) */
};

/* Model topology.  Mirrors the [neural_receiver] block of the reference cfg
 * (config/nrx_rt.cfg:57-75) plus [system] num_rx_antennas / mcs_index.  Everything nrx_create
 * accepts runs every schedule of both precisions (tests/test_gpu_topologies.py: 1, 3, 4, 6, 8, 9
 * antennas, 1..8 bits, 3 heads / 8 masked MCS, with and without h_hat, 1..16 users); a topology
 * outside the ranges below is refused with NRX_ERR_UNSUPPORTED. */
typedef struct nrx_desc {
  int32_t num_rx_ant;        /* A, 1..16 (odd A included) */
  int32_t d_s;               /* state width; kernels are built for 56 */
  int32_t num_it;            /* trained CGNN iterations (len(iterations)) */
  int32_t num_mcs;           /* M = len(mcs_index), 1..8 with var_mcs_masking, 1..3 without */
  int32_t bits[8];           /* bits per symbol of each MCS, 1..8 */
  int32_t var_mcs_masking;   /* 1: one StateInit + one LLR head of max(bits), sliced */
  int32_t init_units[2];     /* num_units_init, kernels built for {128,128} */
  int32_t agg_units;         /* num_units_agg[i] = [64] */
  int32_t state_units[2];    /* num_units_state[i] = [128,128] */
  int32_t readout_units;     /* num_units_readout = [128] */
  int32_t use_h_hat;         /* 1: StateInit consumes h_hat (initial_chest = "ls") */
} nrx_desc;

typedef struct nrx_shape {
  int32_t batch;             /* B slots */
  int32_t num_tx;            /* U users (DMRS ports), 1..16 */
  int32_t num_subcarriers;   /* F = 12 * PRBs */
  int32_t num_symbols;       /* T, must be 14 */
} nrx_shape;

typedef struct nrx_io {
  nrx_shape shape;
  int32_t num_it;            /* iterations to run, 1..desc.num_it (CGNN.num_it setter) */
  int32_t precision;         /* enum nrx_precision */
  const float* y;
  const float* pe;
  const float* h_hat;        /* may be NULL only if desc.use_h_hat == 0 */
  const float* active;
  const float* mcs_mask;     /* may be NULL: treated as one-hot on MCS 0 */
  float* llr;
  float* h_ref;              /* may be NULL */
} nrx_io;

typedef struct nrx_handle nrx_handle;

/* Create an engine on `device` from weights in Keras get_weights() order
 * (the reference loads the same list with
 * utils/utils.py:53-70 load_weights).  `weight_sizes[i]` is the element count of
 * weights[i] and is validated against the topology.  Weights are host pointers;
 * they are copied, converted and packed into device buffers. */
int nrx_create(const nrx_desc* desc, const float* const* weights, const int64_t* weight_sizes,
               int32_t num_weights, int32_t device, nrx_handle** out);

/* Number of weight arrays and the element count of array i for a topology. */
int nrx_weight_layout(const nrx_desc* desc, int32_t* num_weights, int64_t* sizes, int32_t cap);

/* Device workspace (bytes) a forward of this shape/precision needs. */
int nrx_workspace_size(const nrx_handle* h, const nrx_shape* shape, int32_t precision,
                       size_t* bytes);

/* Asynchronous forward on `stream` (hipStream_t; NULL = default stream).
 * All pointers in `io` and `workspace` are device pointers.  No allocation, no host
 * synchronisation: the call can be captured into a hipGraph. */
int nrx_forward(nrx_handle* h, const nrx_io* io, void* workspace, size_t workspace_bytes,
                void* stream);

void nrx_destroy(nrx_handle* h);

/* Input layouts of y for nrx_forward_ex (the wrappers' own input tensors, so that a
 * wrapper call launches only libnrx kernels: no host-framework transpose/concat). */
enum nrx_y_layout {
  NRX_Y_CGNN = 0,       /* io->y [B][F][T][2A] f32, as nrx_forward */
  NRX_Y_SIONNA_RG = 1,  /* io->y = the resource grid [B][1][A][T][F] complex64 (re, im
                           interleaved floats), as CGNNOFDM.forward receives it
                           (neural_rx.py:813-833: y[:,0].permute(0,3,2,1), cat(real, imag)) */
  NRX_Y_SPLIT = 2       /* io->y = rx_slot_real [B][F][T][A], y_imag = rx_slot_imag, as
                           NeuralReceiverONNX.forward (neural_rx.py:1787) */
};

/* Workspace of nrx_forward_ex: nrx_workspace_size plus the CGNN-layout copy of y. */
int nrx_workspace_size_ex(const nrx_handle* h, const nrx_shape* shape, int32_t precision, int32_t y_layout,
                          size_t* bytes);

/* nrx_forward with y in one of the layouts above (y_imag: NRX_Y_SPLIT only, else NULL).
 * The other tensors of `io` keep their nrx_forward layouts. */
int nrx_forward_ex(nrx_handle* h, const nrx_io* io, int32_t y_layout, const float* y_imag, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- Aerial contract
 * The NeuralReceiverONNX / TensorRT engine I/O (neural_rx.py:1773-1812; feed dict of
 * notebooks/real_time_nrx.ipynb:792-844): LS channel estimates at the DMRS pilots in, the
 * FOCC removal + per-PRB nearest-pilot interpolation + positional encoding
 * (NRPreprocessing, neural_rx.py:1614-1711) run on the GPU, LLRs out in the Aerial layout
 * and sign.  Single MCS, as the ONNX export (LLR head 0, mcs mask one-hot on MCS 0).
 *   y_real, y_imag        [B][F][T][A]            f32   rx_slot_{real,imag}
 *   h_ls_real, h_ls_imag  [B][Npil][U][A]         f32   LS estimates at the pilots,
 *                          Npil = nsym * (F/12) * npil, pilot p = (k * F/12 + prb) * npil + j
 *                          (DMRS symbol k, PRB, pilot j of the PRB); FOCC pairs p, p^1
 *   dmrs_port_mask        [B][U]                  f32   active DMRS ports
 *   dmrs_ofdm_pos         [U][nsym]               i32   DMRS symbol indices (device)
 *   dmrs_subcarrier_pos   [U][npil]               i32   pilot subcarriers within a PRB (device)
 *   llr                   [B][bits][U][F][T]      f32   out, LLR = log p(b=0)/p(b=1)
 *   h_hat                 [B][U][F][T][2A]        f32   out, refined estimate (NULL: skip)
 * The contents of dmrs_ofdm_pos / dmrs_subcarrier_pos are device data the host never reads
 * and are not validated: the caller keeps every entry inside 0..13 / 0..11 (any order,
 * per user).  Entries outside that range are not a memory hazard (they only enter
 * distances) but give a preprocessing the reference does not define.
 */
typedef struct nrx_aerial_io {
  nrx_shape shape;           /* B, U = num_tx, F (multiple of 12), T = 14 */
  int32_t num_it;
  int32_t precision;
  int32_t num_dmrs_symbols;  /* nsym */
  int32_t num_dmrs_subcarriers; /* npil (even; 6 for DMRS type 1) */
  const float* y_real;
  const float* y_imag;
  const float* h_ls_real;
  const float* h_ls_imag;
  const float* dmrs_port_mask;
  const int32_t* dmrs_ofdm_pos;
  const int32_t* dmrs_subcarrier_pos;
  float* llr;
  float* h_hat;
} nrx_aerial_io;

/* Workspace of nrx_forward_aerial (the CGNN workspace plus the preprocessed y, h_hat, pe,
 * NN table and the Sionna-layout LLRs). */
int nrx_aerial_workspace_size(const nrx_handle* h, const nrx_aerial_io* io, size_t* bytes);

/* Asynchronous Aerial-contract forward on `stream`; device pointers, no allocation, no
 * host synchronisation. */
int nrx_forward_aerial(nrx_handle* h, const nrx_aerial_io* io, void* workspace, size_t workspace_bytes,
                       void* stream);

/* The preprocessing of nrx_forward_aerial alone (the same two launches, through the same
 * internal helper), into caller buffers:
 * y [B][F][T][2A], h_hat [B][U][F][T][2A], pe [U][F][T][2], nn [U][T][12] (index into the
 * per-PRB pilot list, i = k * npil + j); reads io->shape, num_dmrs_*, y_*, h_ls_*, dmrs_*_pos;
 * ignores llr, h_hat, dmrs_port_mask, num_it, precision.  No workspace.  Asynchronous on
 * `stream`. */
int nrx_aerial_preprocess(const nrx_handle* h, const nrx_aerial_io* io, float* y, float* h_hat,
                          float* pe, int32_t* nn, void* stream);

/* Coded-bit layout of one LLR head (Sionna sign): out[B][U][n_data * bits] with
 * out[b][u][i * bits + k] = llr[b][u][f][t][k] for the i-th data RE, data_re[i] = t * F + f
 * in resource-grid order (symbol-major) -- the ResourceGridDemapper + flatten of
 * CGNNOFDM.forward (neural_rx.py:843-852) and DataEvaluator.post_process_llrs
 * (onnx_utils.py:473-516).  `llr` points at head h of the nrx_forward output
 * ([B][U][F][T][bits_stride]); data_re is a device array.  Asynchronous on `stream`. */
int nrx_llr_demap(const float* llr, int32_t batch, int32_t num_tx, int32_t num_subcarriers,
                  int32_t num_symbols, int32_t bits_stride, int32_t bits, const int32_t* data_re,
                  int32_t n_data, float* out, void* stream);

/* ---------------------------------------------------------------- slot generator
 * Seeded synthetic PUSCH slots generated on the GPU -- replaces the
 * transmitter + channel + LS-estimator chain of E2E_Model.forward (utils/e2e_model.py:
 * 219-344: random active DMRS ports 187-193, x *= active 311-313, Eb/N0 -> no 323-332)
 * for evaluation loops that never leave the device.  The algorithm (Philox4x32-10 draws
 * keyed by seed and counted by the global slot index slot_offset + b, Gray QAM / DMRS type
 * 1 QPSK x sqrt(2), tapped-delay-line channel with exponential PDP and sum-of-sinusoids
 * Doppler, AWGN, LS at the nearest own pilot) is stated in oracle/synth_ref.py. */
typedef struct nrx_gen_desc {
  int32_t batch;               /* B slots in this call */
  int32_t num_tx;              /* U DMRS ports, 1..16 */
  int32_t num_subcarriers;     /* F */
  int32_t num_symbols;         /* T, must be 14 */
  int32_t num_rx_ant;          /* A, 1..16 */
  int32_t num_dmrs_symbols;    /* 1..4 */
  int32_t dmrs_symbols[4];     /* ascending */
  int32_t dmrs_symbol_mask;    /* bit t set <=> t is a DMRS symbol (no data) */
  int32_t cdm_group[16];       /* per port, 0/1 (DMRS type 1: even / odd subcarriers) */
  int32_t num_mcs;             /* M, 1..8 */
  int32_t mcs_bits[8];         /* bits per symbol of each MCS: 2, 4 or 6 */
  int32_t mcs_of_user[16];     /* MCS index per port, -1 = drawn per slot */
  int32_t num_active;          /* active ports per slot (1..U), placed at random */
  int32_t num_taps;            /* TDL taps, 1..8 */
  int32_t num_sinusoids;       /* Doppler sinusoids per tap, 1..16 */
  int32_t pad_;
  double max_delay_s;
  double max_doppler_hz;
  double subcarrier_spacing;   /* Hz */
  double no;                   /* noise variance per RE (complex) */
  uint64_t seed;
  int64_t slot_offset;         /* global index of slot 0 of this call */
} nrx_gen_desc;

/* Device outputs; any pointer except y may be NULL. */
typedef struct nrx_gen_out {
  float* y;                    /* [B][F][T][2A] (nrx_io.y layout) */
  float* h_hat;                /* [B][U][F][T][2A] LS + nearest-neighbour */
  float* h;                    /* [B][U][F][T][2A] true channel */
  float* active;               /* [B][U] */
  float* mcs_mask;             /* [B][U][M] one-hot (nrx_io.mcs_mask) */
  uint8_t* mcs;                /* [B][U] MCS index */
  uint8_t* bits;               /* [B][U][F][T][bits_stride], 0 on DMRS REs and k >= bits */
  int32_t bits_stride;         /* >= max(mcs_bits) */
  int32_t pad_;
  float* y_real;               /* [B][F][T][A] Aerial rx_slot_real */
  float* y_imag;
  float* h_ls_real;            /* [B][Npil][U][A] Aerial LS pilots (nrx_aerial_io), needs F % 12 == 0 */
  float* h_ls_imag;
} nrx_gen_out;

int nrx_gen_workspace_size(const nrx_gen_desc* desc, size_t* bytes);
int nrx_generate_slots(const nrx_gen_desc* desc, const nrx_gen_out* out, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Per-user channel profiles and receive-antenna correlation: the parts of the reference's
 * evaluation channel that its own text defines (utils/channel_models.py:39-161, "DoubleTDL":
 * every user its own delay spread and Doppler; gnb_correlation_matrix, 20-33).  The 3GPP tap
 * tables are not reconstructed: the taps stay the generator's random ones.
 *   - port u draws its delays and its PDP constant from max_delay_s[u] and its Doppler
 *     frequencies from max_doppler_hz[u]; the scalars of nrx_gen_desc are not read.  The Philox
 *     streams and counters are those of nrx_generate_slots.
 *   - rx_mix = M mixes the finished taps (PDP scaling included) over the antennas,
 *     g'[a] = sum_a' M[a][a'] g[a'] in complex f64 with a' ascending, in place in the workspace
 *     (nrx_gen_workspace_size is unchanged), so the taps have the spatial covariance M M^H and
 *     h, y, h_hat and the Aerial outputs all follow from the mixed taps.  The host side
 *     (neural_rx_amd/generator.py) passes the Hermitian square root of a correlation matrix.
 * chan == NULL is exactly nrx_generate_slots; a chan whose first U entries equal the desc's
 * scalars with rx_mix == NULL gives bit-identical outputs to it.  Entries of ports >= U are not
 * read.  Slot slot_offset + b stays a pure function of the global slot index.  A negative or
 * non-finite spread of a port < U, or an rx_mix that is not 8-byte aligned, is
 * NRX_ERR_INVALID_ARG; the other checks are those of
 * nrx_generate_slots, and all are made before the first HIP call. */
typedef struct nrx_gen_chan {
  double max_delay_s[16];      /* per port, >= 0, replaces nrx_gen_desc.max_delay_s for that port */
  double max_doppler_hz[16];   /* per port, >= 0, replaces nrx_gen_desc.max_doppler_hz */
  const double* rx_mix;        /* device, [A][A][2] (re, im), row-major M; NULL = identity */
} nrx_gen_chan;

int nrx_generate_slots_ex(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_out* out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- carrier frequency offset
 * A per-user carrier frequency offset (CFO) at the transmitter: the reference's cfo_offset_ppm(_eval)
 * (utils/impairments.py:18-110, applied at utils/e2e_model.py:320-321), a uniform draw in +-max per
 * (slot, user).  With scs = subcarrier_spacing, kappa = 1.07 the generator's symbol-time factor, N the
 * FFT size and eps[b][u] the offset in subcarrier spacings:
 *   eps[b][u] = cfo_hz[u] / scs                           (constant)
 *             = (cfo_hz[u] / scs) (2 uni(w) - 1)           (otherwise; w = word 0 of the Philox draw
 *               (slot, stream 6, element u): a stream of its own, so no other draw moves)
 *   x'[b,u,k,t] = e^{j theta_t} sum_{m < F} c[m - k] x[b,u,m,t]
 *   c[d]    = D_N(d + eps),  D_N(v) = e^{j pi (N - 1) v / N} sin(pi v) / (N sin(pi v / N)),
 *             D_N(v) = 1 where v / N is an integer
 *   theta_t = 2 pi eps (kappa t + (kappa - 1))
 * which is OFDM modulation with a cyclic prefix of (kappa - 1) N samples, a rotation of sample n by
 * e^{j 2 pi (eps / N) n}, and demodulation; leakage outside the F allocated subcarriers is dropped.
 * With N = F the map is circulant and unitary.  The channel acts on x' (y, h_hat and the Aerial
 * outputs follow from it); the LS step still divides by the clean pilot.  All of it in f64.
 *   - h_with_phase = 0: h stays the channel alone, the reference's perfect CSI.
 *     h_with_phase = 1: h is the diagonal of the effective channel, h e^{j theta_t} D_N(eps) --
 *     what a perfect-CSI receiver and a channel NMSE should be scored against (the f32 h is
 *     multiplied in f64 and rounded once more).
 *   - eps_out (optional, device [B][U] f64, 8-byte aligned) receives eps of every (slot, user),
 *     active or not.
 * cfo == NULL, or every cfo_hz[u] with u < U equal to 0, launches nothing new, needs the workspace
 * of nrx_gen_workspace_size and gives outputs bit-identical to nrx_generate_slots_ex (eps_out is
 * then not written).  Otherwise the workspace grows by the x' buffer [B][U][F][14] complex f64
 * (nrx_gen_workspace_size_cfo).  Slot slot_offset + b stays a pure function of the global slot
 * index; no atomics, the same bits on every call.
 * A negative or non-finite cfo_hz[u] with u < U, constant or h_with_phase outside {0, 1}, or an
 * eps_out that is not 8-byte aligned is NRX_ERR_INVALID_ARG; fft_size non-zero and outside F..8192
 * is NRX_ERR_SHAPE; entries of ports >= U are not read; the other checks are those of
 * nrx_generate_slots_ex, all made before the first HIP call. */
typedef struct nrx_gen_cfo {
  double cfo_hz[16];           /* per port, finite and >= 0: the offset (constant) or its maximum */
  int32_t constant;            /* 0: drawn per (slot, user) in +-cfo_hz[u]; 1: exactly cfo_hz[u] */
  int32_t fft_size;            /* N; 0 = F (the PUSCH grid without guard carriers), else F..8192 */
  int32_t h_with_phase;        /* 0 / 1 */
  int32_t pad_;
  double* eps_out;             /* device [B][U], or NULL */
} nrx_gen_cfo;

int nrx_gen_workspace_size_cfo(const nrx_gen_desc* desc, const nrx_gen_cfo* cfo, size_t* bytes);
int nrx_generate_slots_cfo(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                           const nrx_gen_out* out, void* workspace, size_t workspace_bytes, void* stream);

/* DMRS-based CFO estimate and compensation on the receiver side.  Both are asynchronous on `stream`,
 * use no atomics and no workspace, and give the same bits on every call and for every batch split.
 *
 * nrx_cfo_estimate: eps[b][u] (f64) from h_in = h_hat, read at the own pilots only (subcarriers f
 * with f mod 2 = cdm_group[u] on the DMRS symbols, as the channel estimators do).  With g the smallest
 * gap between consecutive DMRS symbols and the sum over the consecutive pairs (D, D + g) with that
 * gap, the antennas a and the own pilots p,
 *   r = sum h_hat[p, D + g, a] conj(h_hat[p, D, a]),   eps = arg(r) / (2 pi kappa g),
 * reduced in f64 in a fixed order, one workgroup per (slot, user); eps = 0 with fewer than two DMRS
 * symbols, r = 0 or an inactive user (active <= 0).  Unambiguous for |eps| < 1 / (2 kappa g): 0.0519,
 * 1.56 kHz, for symbols (2, 11) at 30 kHz.  A per-tap Doppler shift common to a user's taps looks
 * like a CFO to this estimator, and it is meant to: both turn the channel between the DMRS symbols,
 * and compensating the common rotation helps either way.  h_out, ref_mode and sign are not read.
 *
 * nrx_cfo_rotate: h_out[b,u,f,t,.] = h_in[b,u,f,t,.] e^{j sign 2 pi kappa eps[b][u] (t - t_ref)},
 * f64 arithmetic rounded once to f32; h_out == h_in is allowed.  ref_mode
 *   NRX_CFO_REF_NEAREST_DMRS  t_ref = the first listed DMRS symbol nearest t (the generator's
 *                             nearest-pilot rule): with sign = +1 it compensates the nearest-neighbour
 *                             h_hat that the CGNN and the LS-NN baselines consume;
 *   NRX_CFO_REF_ZERO          t_ref = 0: sign = -1 de-rotates the pilots before nrx_chest_lin /
 *                             nrx_chest_lmmse / nrx_chest_lmmse3, sign = +1 re-rotates their output.
 * active and cdm_group are not read.
 *
 * A NULL io / h_in / eps (estimate: or active; rotate: or h_out), an eps that is not 8-byte aligned,
 * a DMRS symbol outside 0..13 or not ascending, a cdm_group outside {0, 1}, and for the rotation a
 * ref_mode outside the two above or a sign other than +-1 is NRX_ERR_INVALID_ARG; the shape limits
 * and codes are those of nrx_chest_io.  Every argument is checked before the first HIP call. */
#define NRX_CFO_REF_NEAREST_DMRS 0
#define NRX_CFO_REF_ZERO 1
typedef struct nrx_cfo_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;   /* B, U (1..16), F (1..3300), T = 14 */
  int32_t num_rx_ant;          /* A, 1..16 */
  int32_t num_dmrs_symbols;    /* nd, 1..4 */
  int32_t dmrs_symbols[4];     /* ascending */
  int32_t cdm_group[16];       /* per port, 0/1 */
  int32_t ref_mode;            /* nrx_cfo_rotate: NRX_CFO_REF_* */
  int32_t sign;                /* nrx_cfo_rotate: +1 / -1 */
  const float* h_in;           /* [B][U][F][T][2A] */
  const float* active;         /* [B][U] (nrx_cfo_estimate) */
  double*      eps;            /* [B][U]: written by nrx_cfo_estimate, read by nrx_cfo_rotate */
  float*       h_out;          /* [B][U][F][T][2A] (nrx_cfo_rotate) */
} nrx_cfo_io;

int nrx_cfo_estimate(const nrx_cfo_io* io, void* stream);
int nrx_cfo_rotate(const nrx_cfo_io* io, void* stream);

/* ---------------------------------------------------------------- cover-coded DMRS ports, LS estimator
 * DMRS ports in the arrangement of DMRS configuration type 1, as this project defines it, and the
 * receiver-side least-squares estimate that despreads them (the step of the reference's
 * NeuralPUSCHReceiver.estimate_channel, neural_rx.py:1462-1514).  tests/dmrs_ref.py states both in
 * numpy float64.
 *
 * Port u is (g, wf, wt) = (cdm_group[u], focc[u], tocc[u]): the comb offset, a frequency cover over
 * the pairs (j, j^1) of comb positions j = f >> 1, and a time cover over the pairs (k, k^1) of
 * positions k in dmrs_symbols.  With r[g][j][k] the base sequence of CDM group g, port u sends
 *   x_u[f, t_k] = active r[g][j][k] (-1)^(wf (j & 1)) (-1)^(wt (k & 1))     on f mod 2 = g, else 0,
 * so the up to 8 ports are orthogonal over a 2 x 2 block of pilots.  The estimate is, with
 * z[j][k][a] = y[f][t_k][a] conj(p) / |p|^2, p = pilots[g][j][k],
 *   h_ls_u[j][k][a] = mean over j' in {j, j^1 if despread_f}, k' in {k, k^1 if despread_t} of
 *                     (-1)^(wf (j' & 1) + wt (k' & 1)) z[j'][k'][a],
 * complex f64 arithmetic on the f32 inputs, rounded once to f32; a port with active <= 0 gives zeros.
 *   h_hat      [B][U][F][T][2A]  h_ls at the port's nearest own pilot: Manhattan distance, first in
 *              the pilot order (subcarrier-major, then DMRS symbol) -- the generator's rule.  A port
 *              without a pilot in the grid (F = 1, group 1) gives zeros.
 *   h_ls_real / h_ls_imag [B][Npil][U][A]  the Aerial pilot list (nrx_aerial_io; Npil = nd F / 2,
 *              p = k F / 2 + j, needs F % 12 == 0): the estimate before frequency despreading,
 *              (-1)^(wf (j & 1)) times the mean over the time pair only, so that the pair average of
 *              nrx_forward_aerial / nrx_aerial_preprocess performs the frequency despreading.
 * Asynchronous on `stream`; no workspace, no atomics, no allocation, no host synchronisation; the
 * same bits on every call and for every batch split.
 *
 * Checks, all before the first HIP call: a NULL io / y / pilots, all three outputs NULL, or only one
 * of h_ls_real / h_ls_imag is NRX_ERR_INVALID_ARG; the shape limits and codes are those of
 * nrx_chest_io; focc / tocc of a port < U or despread_f / despread_t outside {0, 1}, two ports < U
 * with the same (g, wf, wt), a port with wf = 1 without despread_f or with wt = 1 without despread_t,
 * and despread_t with an odd num_dmrs_symbols or a pair that is not (t, t + 1) are
 * NRX_ERR_INVALID_ARG; despread_f with F % 4 != 0 and the Aerial list with F % 12 != 0 are
 * NRX_ERR_SHAPE.  Entries of ports >= U are not read. */
typedef struct nrx_ls_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;   /* B, U (1..16), F (1..3300), T = 14 */
  int32_t num_rx_ant;          /* A, 1..16 */
  int32_t num_dmrs_symbols;    /* nd, 1..4 */
  int32_t dmrs_symbols[4];     /* ascending */
  int32_t cdm_group[16];       /* per port, 0/1 */
  int32_t focc[16];            /* per port, 0/1: frequency cover */
  int32_t tocc[16];            /* per port, 0/1: time cover */
  int32_t despread_f;          /* 0/1: average the frequency pair (needs F % 4 == 0) */
  int32_t despread_t;          /* 0/1: average the time pair (needs DMRS symbols in pairs t, t + 1) */
  const float* y;              /* [B][F][T][2A] */
  const float* pilots;         /* [2][Pmax][nd][2] (re, im), Pmax = (F + 1) / 2; any non-zero values */
  const float* active;         /* [B][U], or NULL = every port active */
  float*       h_hat;          /* [B][U][F][T][2A], or NULL */
  float*       h_ls_real;      /* [B][Npil][U][A], or NULL (with h_ls_imag) */
  float*       h_ls_imag;
} nrx_ls_io;

int nrx_ls_estimate(const nrx_ls_io* io, void* stream);

/* The slot generator with such ports.  The base sequence is r[g][j][k] = s0 + j s1 with
 * s = 1 - 2 bit, bits 0 and 1 of word 0 of the Philox draw (slot 0, stream 7, element
 * (g Pmax + j) 4 + k): amplitude sqrt(2), a function of the seed alone -- not of the slot or the user
 * -- and a stream of its own, so no other draw moves.  It is this project's sequence, not the Gold
 * sequence of TS 38.211.
 * dmrs == NULL is exactly nrx_generate_slots_cfo: the same launches, workspace and bits.  With a
 * dmrs, the pilots of port u are x_u above with cdm_group from the desc; data REs, bits, mcs, active,
 * h and the noise keep their draws, so y differs on the DMRS symbols only; h_hat and the Aerial
 * list come from the device code of nrx_ls_estimate, run on the generator's y, pilot table and active
 * mask (bit-equal to that call); pilots_out (optional, device [2][Pmax][nd][2] f32) receives the
 * table.  The workspace grows by the table (nrx_gen_workspace_size_dmrs).  The port checks are those
 * of nrx_ls_estimate, the others those of nrx_generate_slots_cfo, all before the first HIP call. */
typedef struct nrx_gen_dmrs {
  int32_t focc[16];            /* per port, 0/1 */
  int32_t tocc[16];            /* per port, 0/1 */
  int32_t despread_f;          /* 0/1, of the generator's own LS outputs */
  int32_t despread_t;
  float* pilots_out;           /* device, or NULL */
} nrx_gen_dmrs;

int nrx_gen_workspace_size_dmrs(const nrx_gen_desc* desc, const nrx_gen_cfo* cfo, const nrx_gen_dmrs* dmrs,
                                size_t* bytes);
int nrx_generate_slots_dmrs(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                            const nrx_gen_dmrs* dmrs, const nrx_gen_out* out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- channel impulse response replay
 * The slot generator on a caller-supplied set of channel impulse responses (CIRs) instead of its own
 * tapped-delay line: the reference's channel_type = "Dataset" (utils/channel_models.py:163-321, the
 * site-specific evaluation).  tests/cir_ref.py states it in numpy f64.
 *   dataset   a [E][A][L][Ta][2] f32 (re, im) path coefficients and tau [E][L] f32 path delays in
 *             seconds, device arrays of the caller: E examples, A = desc.num_rx_ant, L paths, Ta = 1
 *             (static over the slot) or 14 (one coefficient per OFDM symbol).
 *   example   of (slot b, user u), by `select`:
 *             0  e = index[b][u] (int32 device [B][U]); a value outside 0..E-1 gives that user a zero
 *                channel and reads nothing of the dataset
 *             1  e = w mod E, w = word 0 of the Philox draw (slot, stream 8, element u): a stream of
 *                its own, so no other draw moves
 *             2  n = E / U, e = U (w mod n) + u: user u stays on the examples that are u modulo U (the
 *                reference's evaluation rule, two interleaved trajectories)
 *   channel   H_u[a, f, t] = sum_{l < L} g_l(t) exp(-j 2 pi ((f + f_offset) subcarrier_spacing) tau[e][l]),
 *             g_l(t) = a[e][a][l][Ta == 1 ? 0 : t]; f64, l ascending, the f32 inputs widened exactly.
 *             f_offset = 0 is the built-in generator's convention, -F / 2 the centred one.
 *   normalize c[b][u] = mean over (a, f, t) of |H_u|^2;  H_u <- H_u / sqrt(c), zeros where c = 0: unit
 *             mean energy per (slot, user) over the grid.  Fixed-order f64 sums, no atomics.
 * Everything behind H is the generator's: y = sum_u H_u x_u + noise with the same noise and x, h for
 * every user, h_hat / the Aerial lists, the CFO (which acts on x) and the cover-coded ports.  bits, mcs
 * and active are bit-equal to a built-in run of the same seed, so curves on the two channels are paired.
 * cir == NULL is exactly nrx_generate_slots_dmrs: the same launches, workspace and bits.  With a cir,
 * chan must be NULL (a dataset brings its own delay, Doppler and antenna structure); the desc's
 * num_taps, num_sinusoids, max_delay_s and max_doppler_hz are validated as always and have no effect.
 * The workspace grows by H in f64 and the energy sums (nrx_gen_workspace_size_cir).  Slot
 * slot_offset + b stays a pure function of the global slot index and the dataset; every output element
 * has one writer; the same bits on every call and for every split of the slots over calls.
 * NRX_ERR_INVALID_ARG: a NULL or not 8-byte aligned a, a NULL tau, a NULL index with select == 0, select
 * outside 0..2, a non-finite f_offset, chan != NULL.  NRX_ERR_SHAPE: num_examples outside 1..2^24,
 * num_paths outside 1..1024 (a validation limit, not a hardware one), num_time_steps not 1 or 14,
 * select == 2 with num_examples < num_tx.  The other checks are those of nrx_generate_slots_dmrs, all
 * before the first HIP call. */
typedef struct nrx_gen_cir {
  int32_t num_examples, num_paths, num_time_steps, select;   /* E, L, Ta (1|14), 0|1|2 */
  int32_t normalize, pad_;
  double  f_offset;
  const float*   a;      /* [E][A][L][Ta][2], 8-byte aligned */
  const float*   tau;    /* [E][L] */
  const int32_t* index;  /* [B][U], select == 0 only */
} nrx_gen_cir;

int nrx_gen_workspace_size_cir(const nrx_gen_desc* desc, const nrx_gen_cfo* cfo, const nrx_gen_dmrs* dmrs,
                               const nrx_gen_cir* cir, size_t* bytes);
int nrx_generate_slots_cir(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                           const nrx_gen_dmrs* dmrs, const nrx_gen_cir* cir, const nrx_gen_out* out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The built-in channel in the dataset's format, to be replayed here or elsewhere: the finished taps of
 * nrx_generate_slots_ex (PDP scaling and rx_mix included) and their delays, rounded once to f32.
 * a_out [B][U][A][L][14][2], tau_out [B][U][L], L = desc.num_taps: a dataset of E = B U examples with
 * Ta = 14, example b U + u.  The workspace is that of nrx_gen_workspace_size; the checks are those of
 * nrx_generate_slots_ex, and a NULL a_out or tau_out is NRX_ERR_INVALID_ARG. */
int nrx_generate_taps(const nrx_gen_desc* desc, const nrx_gen_chan* chan, float* a_out, float* tau_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- OFDM modulation and demodulation
 * The step between time-domain samples and the resource grid that everything else here consumes: the
 * reference's OFDMModulator / OFDMDemodulator (utils/siona_tf.py:4407-4643) with its unitary fft / ifft
 * (4331-4402, scale 1 / sqrt(N) each way).  tests/ofdm_ref.py states both in numpy.
 *
 * N = fft_size, F = grid_subcarriers, bin(f) = (f + first_bin - N/2) mod N: first_bin is the position of
 * grid subcarrier 0 on the fftshifted axis (DC in the middle), the default N/2 - F/2 centres the grid.
 * The sample row of stream (b, s) holds the symbols back to back, symbol t at
 * start[t] = sum over t' < t of (cp_length[t'] + N); entries of cp_length at t >= T are not read.
 *
 * nrx_ofdm_modulate, per (b, s, t): grid subcarrier f goes to bin(f), the other bins are zero; the unitary
 * IDFT; the last cp_length[t] samples are prepended; the symbols are concatenated.  With pa_asat = A > 0
 * a sample v is stored as the Rapp curve v / (1 + (|v| / A)^(2p))^(1 / (2p)), p = pa_smoothness, evaluated
 * in f64; pa_asat <= 0 is the linear amplifier.  Samples from the end of symbol T - 1 up to L are written
 * zero: every element of `samples` is written.  timing_advance and offset are not read.
 *
 * nrx_ofdm_demodulate: the window of symbol t of stream s starts at sample
 *   offset[s] + start[t] + cp_length[t] - timing_advance;
 * samples outside [0, L) read as zero.  The unitary DFT; bin k (unshifted, 0..N-1) is multiplied by
 * e^{+j 2 pi k timing_advance / N}; bin(f) is written to grid subcarrier f.  With F = N, first_bin = 0, a
 * uniform cyclic prefix and zero offsets this is OFDMDemodulator(N, l_min = -timing_advance, cp) on a
 * sequence that already starts at l_min.  Every element of `grid` is written.  pa_* are not read; entries
 * of offset at s >= S are not read.
 *
 * One launch each: a transform lives in LDS between its one global read and its one global write
 * (csrc/nrx_ofdm.hip).  Asynchronous on `stream`; no workspace, no atomics; the same bits on every call
 * and for every split of the batch.  (The F of this struct is grid_subcarriers, not num_subcarriers: that name
 * belongs to the slot grids [batch][num_tx][num_subcarriers][14], and this one has streams and 1..14 symbols.)
 *
 * Checks, all before the first HIP call.  NRX_ERR_INVALID_ARG: a NULL io / grid / samples, an unknown
 * precision or grid_layout, a grid or samples pointer not aligned to its complex element (8 bytes f32, 16
 * bytes f64; a CGNN grid to its real element), modulate with pa_asat > 0 and a pa_smoothness that is not
 * finite and > 0.  NRX_ERR_SHAPE: fft_size not a power of two in 64..4096, B outside 1..65535, S outside
 * 1..16, T outside 1..14, F outside 1..N, first_bin outside -1..N-F, a cp_length outside 0..N, demodulate
 * with timing_advance outside 0..min cp_length, num_samples < start[T]. */
#define NRX_OFDM_F32 0
#define NRX_OFDM_F64 1
#define NRX_OFDM_GRID_PLANAR 0   /* [B][S][F][T] complex (re, im): the generator's x / x' layout */
#define NRX_OFDM_GRID_CGNN   1   /* [B][F][T][2S], Re s0..s(S-1) then Im s0..: nrx_io.y */
typedef struct nrx_ofdm_io {
  int32_t batch, num_streams, grid_subcarriers, num_symbols; /* B 1..65535, S 1..16, F 1..N, T 1..14 */
  int32_t fft_size;        /* N: a power of two, 64..4096 */
  int32_t first_bin;       /* fftshifted index of grid subcarrier 0, 0..N-F; -1 = N/2 - F/2 (floor) */
  int32_t cp_length[14];   /* per symbol, 0..N */
  int32_t precision;       /* NRX_OFDM_F32 / _F64: element type of grid AND samples */
  int32_t grid_layout;
  int32_t timing_advance;  /* demodulate: d = -l_min, 0..min(cp_length) */
  int32_t offset[16];      /* demodulate, per stream: added to every window start; may be negative */
  int64_t num_samples;     /* L: samples per (b, s) row, >= sum_t (cp_length[t] + N) */
  double  pa_asat;         /* modulate: Rapp saturation amplitude; <= 0 = linear */
  double  pa_smoothness;   /* modulate: p > 0, read only when pa_asat > 0 */
  void*   grid;
  void*   samples;         /* [B][S][L] complex (re, im) */
} nrx_ofdm_io;

int nrx_ofdm_modulate(const nrx_ofdm_io* io, void* stream);
int nrx_ofdm_demodulate(const nrx_ofdm_io* io, void* stream);

/* The slot generator with a time-domain transmit stage: x' = demodulate(impair(modulate(x))) between the
 * transmit grid and the channel, the construction of the reference's hardware-impairment layer
 * (utils/impairments.py:67-108), for the two transmit-side effects without a closed form on the grid:
 *   - a power-amplifier non-linearity: the Rapp curve above with A = sqrt(F / N) 10^(pa_ibo_db / 20), an
 *     input back-off over the nominal mean sample power F / N of the unit-energy grid; no
 *     re-normalisation after compression, as with an amplifier at a fixed drive;
 *   - a timing error per port: delay[u] >= 0 samples, that user's signal arrives this late.  The receive
 *     windows stay where they are (offset[u] = -delay[u], timing_advance = 0), so a delay inside the
 *     cyclic prefix is the frequency ramp e^{-j 2 pi delay k_f / N}, k_f = f + first_bin - N/2 (signed), and
 *     one beyond it adds inter-symbol and inter-carrier interference; symbol 0 reads zeros before the row.
 * All of it in f64 (NRX_OFDM_F64, the PLANAR layout).  The channel acts on x'; y, h_hat and the Aerial
 * outputs follow from it; the LS step still divides by the clean pilot; bits, active ports, MCS and noise
 * keep their draws, so curves with and without the stage are paired.
 *   - h_with_delay = 1 multiplies h[b,u,f,t] by e^{-j 2 pi delay[u] k_f / N}: the exact effective channel for
 *     a delay inside the cyclic prefix and the dominant term beyond it (f64 arithmetic on the f32 h,
 *     rounded once more).  0 leaves h the channel alone.
 *   - x_out (optional, device [B][U][F][14] complex f64, 8-byte aligned) receives x' of every (slot, user).
 * td == NULL is exactly nrx_generate_slots_cir: nothing new is launched, the workspace and the bits are the
 * same.  Otherwise the workspace grows by x' and the sample buffer [B][U][L] complex f64, L = sum_t
 * (cp_length[t] + N) (nrx_gen_workspace_size_td): about 250 MB at B = 128, U = 2, N = 4096.  Slot
 * slot_offset + b stays a pure function of the global slot index; no atomics, the same bits on every call.
 * NRX_ERR_INVALID_ARG: a td together with a cfo that has a non-zero offset (one transmit-side stage per
 * call), a negative delay of a port < U, pa_enable or h_with_delay outside {0, 1}, with pa_enable a
 * non-finite pa_ibo_db or a pa_smoothness that is not finite and > 0, an x_out that is not 8-byte aligned.
 * NRX_ERR_SHAPE: fft_size, first_bin and cp_length as for nrx_ofdm_io with F = num_subcarriers.  The other
 * checks are those of nrx_generate_slots_cir, all before the first HIP call. */
typedef struct nrx_gen_td {
  int32_t fft_size, first_bin;   /* as nrx_ofdm_io; F <= N */
  int32_t cp_length[14];
  int32_t delay[16];             /* per port, samples, >= 0: that user's signal arrives this late */
  int32_t pa_enable;             /* 0 / 1 */
  int32_t h_with_delay;          /* 0 / 1 */
  double  pa_ibo_db;             /* input back-off over the nominal mean sample power F/N */
  double  pa_smoothness;
  double* x_out;                 /* optional, device [B][U][F][14] complex f64: x' of every (slot, user) */
} nrx_gen_td;

int nrx_gen_workspace_size_td(const nrx_gen_desc* desc, const nrx_gen_cfo* cfo, const nrx_gen_dmrs* dmrs,
                              const nrx_gen_cir* cir, const nrx_gen_td* td, size_t* bytes);
int nrx_generate_slots_td(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                          const nrx_gen_dmrs* dmrs, const nrx_gen_cir* cir, const nrx_gen_td* td,
                          const nrx_gen_out* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- Time-domain channel
 * The channel on the samples between OFDM modulation and demodulation: discrete-time taps from the path
 * delays, applied per sample, with path gains that move inside a symbol -- the counterpart of Sionna's
 * TimeChannel, and an addition of this project (the reference's OFDMChannel, utils/parameters.py:346-439,
 * never leaves the frequency domain).  tests/timechan_ref.py states it in numpy.  With fs = sample_rate,
 * sinc(0) = 1, sinc(v) = sin(pi v) / (pi v) and x read as zero outside [0, num_samples):
 *
 *   r[b,a,n] = sum_u sum_l g[b,u,a,l](n) v[b,u,l](n)
 *   g(n)     = sum_{s < NS} g0[b,u,a,l,s] exp(j 2 pi fd[b,u,a,l,s] (n - n0) / fs)
 *   v(n)     = sum_{l' = l_min..l_max} sinc(l' - tau[b,u,l] fs) x[b,u,n - l']
 *
 * and, with rx_mix = M, r'[a] = sum_a' M[a][a'] r[a'] (a' ascending).  The sinc is plainly truncated to
 * l_min..l_max: no window and no re-normalisation, so the energy of a path is preserved only approximately
 * (exactly for a delay of a whole number of samples inside the span; a fractional delay loses the tails beyond
 * the span, of the order 1 / (pi^2 d) of the path's energy at d samples from the nearest end).
 *
 * One launch (csrc/nrx_timechan.hip).  Every element of r is written.  Asynchronous on `stream`; no workspace,
 * no atomics, no allocation, no host synchronisation; the same bits on every call and for every split of the
 * batch: a sinusoid's rotation is exact at a fixed sample stride that depends on num_rx_ant alone.
 *
 * Checks, all before the first HIP call.  NRX_ERR_INVALID_ARG: a NULL io / tau / g0 / fd / x / r, a g0, x, r or
 * rx_mix not 16-byte aligned, a tau or fd not 8-byte aligned, a sample_rate that is not finite and > 0.
 * NRX_ERR_SHAPE: batch outside 1..65535, num_tx or num_rx_ant outside 1..16, num_paths outside 1..8,
 * num_sinusoids outside 1..16, l_min outside -255..0, l_max outside 0..255, l_max - l_min + 1 > 256,
 * num_samples outside 1..2^31 - 1, n0 outside -2^31..2^31 - 1. */
typedef struct nrx_tc_io {
  int32_t batch, num_tx, num_rx_ant, num_paths, num_sinusoids; /* B, U, A, L, NS */
  int32_t l_min, l_max;    /* l_min <= 0 <= l_max, l_max - l_min + 1 <= 256 */
  int32_t pad_;
  int64_t num_samples;     /* Ls: samples per (b, u) row of x and per (b, a) row of r */
  int64_t n0;              /* the sample at which every sinusoid has the phase of its g0 */
  double  sample_rate;     /* fs, Hz */
  const double* tau;       /* device [B][U][L], seconds */
  const double* g0;        /* device [B][U][A][L][NS][2] (re, im) */
  const double* fd;        /* device [B][U][A][L][NS], Hz */
  const double* x;         /* device [B][U][Ls][2] */
  const double* rx_mix;    /* optional, device [A][A][2] */
  double* r;               /* device [B][A][Ls][2] */
} nrx_tc_io;

int nrx_time_channel(const nrx_tc_io* io, void* stream);

/* The slot generator with the time-domain channel in place of the per-RE product.
 *   - Samples: the modulated x of every (slot, port) (nrx_ofdm_modulate, f64, PLANAR), fs = fft_size scs.
 *   - Channel: nrx_time_channel with the built-in channel's own draws: tau, the sinusoid amplitudes g0 with
 *     sqrt(pdp) folded in, the Doppler frequencies fd, per-port profiles and rx_mix of nrx_gen_chan included.
 *     n0 = cp_length[0], so the useful part of symbol t starts at about t 1.07 / scs, the instant at which the
 *     grid channel samples its gains; each path also carries exp(+j 2 pi (first_bin - N/2) scs tau_l), which
 *     refers the delay ramp to grid subcarrier 0 as on the grid channel.  With zero Doppler the slot is the
 *     realisation of the plain generator up to the sinc truncation, so curves with and without are paired.
 *   - Receive side: the A antenna streams are demodulated with timing_advance = ta; the generator's grid
 *     noise (the same draws) is added after demodulation, where the unitary DFT keeps it white; h_hat and the
 *     Aerial lists come from y as always; bits, active ports and MCS keep their draws.
 *   - h is the ISI-free diagonal of the effective channel, what perfect CSI and the NMSE are scored against:
 *       h[b,u,f,t,a] = sum_l' hbar_t[l'] exp(-j 2 pi k_f l' / N),   k_f = f + first_bin - N/2
 *       hbar_t[l']   = (1/N) sum_{m < N} h_{u,a}[w_t + m, l'],      w_t = start[t] + cp_length[t] - ta
 *       h_{u,a}[n,l'] = sum_l g(n) sinc(l' - tau_l fs)
 *     It is exact when l_max <= cp_length - ta and ta >= -l_min, and the dominant term otherwise: a delay
 *     beyond the prefix adds inter-symbol, a gain that moves inside the window inter-carrier interference.
 *   - l_max < 0 stands for ceil(max over ports of max_delay_s fs) + 6; the usual l_min is -6.
 *   - r_out (optional, device [B][A][Ls] complex f64, Ls = sum_t (cp_length[t] + N)) receives the noise-free
 *     received samples, x_out (optional, device [B][U][Ls] complex f64) the transmitted ones.
 * tc == NULL is exactly nrx_generate_slots_td: the same launches, workspace and bits.  Cover-coded DMRS ports
 * (dmrs) compose: they act on x.  The workspace grows by both sample buffers, the sinusoids and the antenna
 * grids (nrx_gen_workspace_size_tc): about 750 MB at B = 128, U = 2, A = 4, N = 4096.  Slot slot_offset + b
 * stays a pure function of the global slot index; no atomics, the same bits on every call.
 * NRX_ERR_INVALID_ARG: a tc together with a td, a cir or a cfo that has a non-zero offset (one sample-domain
 * stage per call), an r_out or x_out that is not 16-byte aligned.  NRX_ERR_SHAPE: fft_size, first_bin and
 * cp_length as for nrx_ofdm_io with F = num_subcarriers, timing_advance outside 0..min cp_length, l_min outside
 * -255..0, a resolved l_max outside 0..255 or a span l_max - l_min + 1 > 256.  The other checks are those of
 * nrx_generate_slots_td, all before the first HIP call. */
typedef struct nrx_gen_tc {
  int32_t fft_size, first_bin;   /* as nrx_ofdm_io; F <= N */
  int32_t cp_length[14];
  int32_t l_min, l_max;          /* taps l_min..l_max; l_max < 0: from the ports' max_delay_s */
  int32_t timing_advance;        /* 0..min(cp_length) */
  int32_t pad_;
  double* r_out;                 /* optional, device [B][A][Ls] complex f64 */
  double* x_out;                 /* optional, device [B][U][Ls] complex f64 */
} nrx_gen_tc;

int nrx_gen_workspace_size_tc(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                              const nrx_gen_dmrs* dmrs, const nrx_gen_cir* cir, const nrx_gen_td* td,
                              const nrx_gen_tc* tc, size_t* bytes);
int nrx_generate_slots_tc(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                          const nrx_gen_dmrs* dmrs, const nrx_gen_cir* cir, const nrx_gen_td* td,
                          const nrx_gen_tc* tc, const nrx_gen_out* out, void* workspace, size_t workspace_bytes,
                          void* stream);

/* The slot generator with one noise variance per slot: the noise of slot b has the variance no_slot[b] per
 * complex resource element where every other call uses desc.no.  Nothing else changes: the draws, the channel,
 * the bits and every stage are those of nrx_generate_slots_tc, so slot slot_offset + b generated with
 * no_slot[b] = x is bit for bit the slot that a call with desc.no = x gives at that global index, in every
 * output (y, h_hat, h, bits, active, mcs and the Aerial outputs).  noise == NULL or no_slot == NULL is exactly
 * nrx_generate_slots_tc: the same launches, workspace (nrx_gen_workspace_size_tc) and bits.
 * no_slot is device data that the host never reads: the caller keeps every entry finite and >= 0 (as for the
 * Aerial position lists, nothing here can check it).  A no_slot that is not 8-byte aligned is
 * NRX_ERR_INVALID_ARG; the other checks are those of nrx_generate_slots_tc, all before the first HIP call. */
typedef struct nrx_gen_noise {
  const double* no_slot;       /* device, [B]: noise variance per complex RE of slot b; NULL: desc.no */
} nrx_gen_noise;

int nrx_generate_slots_no(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                          const nrx_gen_dmrs* dmrs, const nrx_gen_cir* cir, const nrx_gen_td* td,
                          const nrx_gen_tc* tc, const nrx_gen_noise* noise, const nrx_gen_out* out, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Uncoded error counters of one batch (sim_ber's counting, scripts/evaluate.py:193-202,
 * with the active-port masking of E2E_Model._mask_active_dmrs, e2e_model.py:195-209):
 * counts[u][0..3] += (bit errors, bits, block errors, blocks) over the active (slot, user)
 * pairs, data REs and the first mcs_bits[mcs[b][u]] bits; hard decision LLR > 0 -> 1; a
 * block is one (slot, user) grid.  Asynchronous on `stream`. */
typedef struct nrx_count_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;
  int32_t num_heads;           /* H heads in llr; head = mcs if H > 1 else 0 */
  int32_t bits_stride;         /* last dim of llr and bits */
  int32_t num_mcs;
  int32_t mcs_bits[8];
  int32_t dmrs_symbol_mask;
  const float* llr;            /* [H][B][U][F][T][bits_stride] (nrx_io.llr) */
  const uint8_t* bits;         /* [B][U][F][T][bits_stride] */
  const uint8_t* mcs;          /* [B][U] or NULL (= 0) */
  const float* active;         /* [B][U] */
  int64_t* counts;             /* [U][4] accumulated (device) */
} nrx_count_io;

int nrx_count_errors(const nrx_count_io* io, void* stream);

/* ---------------------------------------------------------------- classical baseline
 * Per-resource-element MIMO LMMSE equaliser + max-log QAM demapper: the detector of the
 * reference's baseline receivers (utils/baseline_rx.py:262-272, LinearDetector("lmmse", "bit",
 * "maxlog"); every cfg sets demapping_type = 'maxlog').  It consumes the generator's tensors as
 * they are (y, and h_hat or the true h as `h`) and writes LLRs in the engine's layout, so the
 * error counters above read them unchanged.  Per RE (b, f, t), with s = no + err_var and H [A x U]
 * the channel whose columns of inactive users (active <= 0) are zero:
 *   G = H^H H + s I,  x^ = G^-1 H^H y,  a_u = (G^-1)_uu,  mu_u = 1 - s a_u,
 *   x~_u = x^_u / mu_u,  nu_u = s a_u / mu_u      (Sionna lmmse_equalizer with whiten_interference:
 *                                                  no_eff = 1 / diag(G H) - 1)
 *   llr[k] = (min_{c: b_k = 0} |x~_u - c|^2 - min_{c: b_k = 1} |x~_u - c|^2) / nu_u,  k < m,
 * over the Gray QAM of TS 38.211 5.1 with m = mcs_bits[mcs[b][u]] bits (the generator's
 * constellation).  Entries k >= m, inactive users, DMRS symbols and RE-users with mu_u < 1e-6 are
 * written exactly 0; every element of llr is written on every call.  f32 arithmetic, no atomics
 * (bit-identical from call to call), no workspace, no allocation, no host synchronisation;
 * asynchronous on `stream`.  Every argument is checked before the first HIP call: a NULL io / y /
 * h / active / llr, no <= 0, err_var < 0 or a bit width outside {2, 4, 6} is NRX_ERR_INVALID_ARG; T != 14,
 * B outside 1..65535, F outside 1..3300, U < 1, A outside 1..16, num_mcs outside 1..8 or bits_stride <
 * max(mcs_bits) is NRX_ERR_SHAPE; U > 8 is NRX_ERR_UNSUPPORTED. */
typedef struct nrx_lmmse_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;   /* B (1..65535), U (1..8), F (1..3300), T = 14 */
  int32_t num_rx_ant;          /* A, 1..16 */
  int32_t bits_stride;         /* last dim of llr, >= max(mcs_bits) */
  int32_t num_mcs;             /* 1..8 */
  int32_t mcs_bits[8];         /* 2, 4 or 6 */
  int32_t dmrs_symbol_mask;    /* bit t set: symbol t carries no data, its LLRs are written 0 */
  int32_t pad_;
  double  no;                  /* noise variance per complex RE, > 0 */
  double  err_var;             /* >= 0, added to no: channel-estimation error power (0 for perfect CSI) */
  const float*   y;            /* [B][F][T][2A]      nrx_io.y layout */
  const float*   h;            /* [B][U][F][T][2A]   h_hat or the true h (nrx_gen_out layouts) */
  const float*   active;       /* [B][U] */
  const uint8_t* mcs;          /* [B][U] or NULL (= 0) */
  float*         llr;          /* [1][B][U][F][T][bits_stride], Sionna sign log p(1)/p(0) */
} nrx_lmmse_io;

int nrx_lmmse_detect(const nrx_lmmse_io* io, void* stream);

/* ---------------------------------------------------------------- K-best detector
 * Near-ML MIMO detection: the detector of the reference's baseline_lmmse_kbest /
 * baseline_perf_csi_kbest systems (utils/baseline_rx.py:242-254, KBestDetector with k = 64).  The
 * reference takes it from Sionna and holds no source of it, so the detector is defined here, and
 * pinned by the exhaustive max-log ML detector where the two must coincide (tests/kbest_ref.py).
 * Stated departures from Sionna's KBestDetector: a real-valued tree (2U levels of PAM) instead of
 * a complex one, a scalar err_var, a Gram-Cholesky instead of a QR, and the ordering and clipping
 * rules below.  Tensors and the LLR layout are those of nrx_lmmse_detect.
 *
 * Per data RE (b, f, t), with s = no + err_var:
 *  1. streams: the n <= U users with active > 0, in port order.  User u has m_u =
 *     mcs_bits[mcs[b][u]] bits of the Gray QAM of TS 38.211 5.1 (the generator's): even bits on the
 *     real axis, odd bits on the imaginary axis, each axis a PAM of L_u = 2^(m_u / 2) levels.
 *  2. real model: y_r = [Re y; Im y] in R^2A; user u has the columns [Re h_u; Im h_u] (for Re x_u)
 *     and [-Im h_u; Re h_u] (for Im x_u).
 *  3. order: users by |h_u|^2 ascending, ties to the lower u; real streams
 *     [Re u(1), Im u(1), Re u(2), Im u(2), ...].  Detection runs from the last stream to the first.
 *  4. G = H_pi^T H_pi (2n x 2n) = R^T R with R upper triangular and a positive diagonal,
 *     y~ = R^-T H_pi^T y_r; no MMSE regularisation.  If a Cholesky pivot d_i <= 1e-6 G_ii, every
 *     LLR of the RE is written 0 (the counterpart of the mu < 1e-6 rule of nrx_lmmse_detect).
 *  5. search: one empty path of metric 0.  At level i = 2n-1 .. 0 every survivor expands into the L
 *     children of that stream, child metric = parent metric + (y~_i - sum_{j>i} R_ij x_j - R_ii a)^2
 *     / s; the k children with the smallest metric survive (all of them while there are at most k).
 *     Children that tie exactly at the k-th place are resolved deterministically.
 *  6. llr[u][q] = clip(min_{p: b_q(p) = 0} metric_p - min_{p: b_q(p) = 1} metric_p, +-llr_clip) over
 *     the final list (Sionna sign, log p(1)/p(0)); a side without a path counts as +inf, so the
 *     result is -+llr_clip.
 * Entries q >= m_u, inactive users and DMRS symbols are written exactly 0; every element of llr is
 * written on every call.  f32 arithmetic, no atomics, no allocation, no host synchronisation;
 * asynchronous on `stream`; bit-identical from call to call and independent of how slots are split
 * into batches.  The workspace (16-byte aligned, nrx_kbest_workspace_size bytes, monotone in B)
 * holds the per-RE Gram matrices between the two kernels.  Every argument is checked before the
 * first HIP call: a NULL io / y / h / active / llr / workspace / bytes, a workspace that is not
 * 16-byte aligned, no <= 0, err_var < 0, llr_clip <= 0, k outside 1..64 or a bit width outside
 * {2, 4, 6} is NRX_ERR_INVALID_ARG; T != 14, B outside 1..65535, F outside 1..3300, U < 1, A
 * outside 1..16, num_mcs outside 1..8 or bits_stride < max(mcs_bits) is NRX_ERR_SHAPE; U > 8 is
 * NRX_ERR_UNSUPPORTED; a workspace smaller than nrx_kbest_workspace_size is NRX_ERR_WORKSPACE. */
typedef struct nrx_kbest_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;   /* B (1..65535), U (1..8), F (1..3300), T = 14 */
  int32_t num_rx_ant;          /* A, 1..16 */
  int32_t bits_stride;         /* last dim of llr, >= max(mcs_bits) */
  int32_t num_mcs;             /* 1..8 */
  int32_t mcs_bits[8];         /* 2, 4 or 6 */
  int32_t dmrs_symbol_mask;    /* bit t set: symbol t carries no data, its LLRs are written 0 */
  int32_t k;                   /* survivors per level, 1..64 */
  double  no;                  /* noise variance per complex RE, > 0 */
  double  err_var;             /* >= 0, added to no: channel-estimation error power (0 for perfect CSI) */
  double  llr_clip;            /* > 0: LLRs are clipped to +-llr_clip */
  const float*   y;            /* [B][F][T][2A]      nrx_io.y layout */
  const float*   h;            /* [B][U][F][T][2A]   h_hat or the true h (nrx_gen_out layouts) */
  const float*   active;       /* [B][U] */
  const uint8_t* mcs;          /* [B][U] or NULL (= 0) */
  float*         llr;          /* [1][B][U][F][T][bits_stride], Sionna sign log p(1)/p(0) */
} nrx_kbest_io;

int nrx_kbest_workspace_size(const nrx_kbest_io* io, size_t* bytes);
int nrx_kbest_detect(const nrx_kbest_io* io, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- channel-estimation baselines
 * The estimators of the reference's baseline_lmmse_lmmse / baseline_lslin_lmmse systems
 * (utils/baseline_rx.py:100-229) and the statistics of its scripts/compute_cov_mat.py, for the
 * generator's channel.  The host side (covariance matrices, filter design) is
 * neural_rx_amd/chest.py.
 *
 * Covariance lag sums of the true channel h [B][U][F][T][2A] (nrx_gen_out.h), over all (b, u)
 * planes, antennas and the other axis, in float64:
 *   acc[d]     += sum_{b,u,a,t} sum_{f < F - d} h[f + d] conj(h[f])      d = 0..F-1   (frequency)
 *   acc[F + d] += sum_{b,u,a,f} sum_{t < 14 - d} h[t + d] conj(h[t])     d = 0..13    (time)
 * acc is a device array double[F + 14][2] (re, im) that the caller zeroes once; every call adds
 * to it, so several batches accumulate.  The caller divides by the product counts
 * B U A 14 (F - d) / B U A F (14 - d) and builds the Hermitian Toeplitz matrices R_f, R_t: the
 * generator's channel is stationary in f and t (oracle/synth_ref.py), so lags estimate what the
 * reference's full matrices estimate, with less variance; its spatial covariance is the identity.
 * f64 products and sums in a fixed order (per-workgroup partial sums in the workspace, then one
 * ordered reduction), no atomics: the same input gives the same bits.  Asynchronous on `stream`.
 * A NULL io / h / acc / workspace / bytes is NRX_ERR_INVALID_ARG; T != 14, B outside 1..65535,
 * U outside 1..16, F outside 1..3300 or A outside 1..16 is NRX_ERR_SHAPE; a workspace smaller than
 * nrx_cov_workspace_size is NRX_ERR_WORKSPACE.  Every argument is checked before the first HIP call. */
typedef struct nrx_cov_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;   /* B, U (1..16), F (1..3300), T = 14 */
  int32_t num_rx_ant;          /* A, 1..16 */
  int32_t pad_;
  const float* h;              /* [B][U][F][T][2A] */
  double*      acc;            /* [F + 14][2], accumulated */
} nrx_cov_io;

int nrx_cov_workspace_size(const nrx_cov_io* io, size_t* bytes);
int nrx_cov_accumulate(const nrx_cov_io* io, void* workspace, size_t workspace_bytes, void* stream);

/* Spatial covariance sums of the true channel, the third matrix of compute_cov_mat.py, for a
 * generator with receive-antenna correlation (nrx_gen_chan.rx_mix), over all (b, u) planes:
 *   acc[a][a'] += sum_{b,u,f,t} h[a] conj(h[a'])
 * acc is a device array double[A][A][2] (re, im) that the caller zeroes once; every call adds to
 * it.  The caller divides by B U F 14.  As in the reference there is one R_s (and one R_f, R_t)
 * for all users: the mixture over the users' profiles.  Same discipline as the lag sums: f64
 * products and sums, a fixed number of per-workgroup partials in the workspace, then one ordered
 * reduction, no atomics, the same bits on every call.  Asynchronous on `stream`.  Error codes
 * and shape limits are those of nrx_cov_accumulate, checked before the first HIP call. */
typedef struct nrx_cov_space_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;   /* B, U (1..16), F (1..3300), T = 14 */
  int32_t num_rx_ant;          /* A, 1..16 */
  int32_t pad_;
  const float* h;              /* [B][U][F][T][2A] */
  double*      acc;            /* [A][A][2], accumulated */
} nrx_cov_space_io;

int nrx_cov_space_workspace_size(const nrx_cov_space_io* io, size_t* bytes);
int nrx_cov_space_accumulate(const nrx_cov_space_io* io, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Channel estimators on the LS estimates at the own pilots.  Both read only the own-pilot REs of
 * h_hat (subcarriers f with f mod 2 = cdm_group[u] on the DMRS symbols; the generator's
 * nearest-neighbour h_hat holds the LS estimate there) and write every element of h_out
 * [B][U][F][T][2A], zeros for inactive users (active <= 0) and for a user without a pilot (F = 1,
 * group 1).  f32, no atomics, no workspace, no allocation, no host synchronisation; asynchronous on
 * `stream`; bit-identical from call to call and independent of how slots are split into batches.
 *
 * nrx_chest_lmmse: the exact 2-D Wiener filter under the separable covariance R_t (x) R_f, from
 * host-designed tables (|P| own pilots, nd DMRS symbols D, k < nd eigen-components of R_t[D, D]):
 *   z_k[p]  = sum_d vconj[k][d] h_ls[P_p, D_d]           vconj[k][d] = conj(v_k[d])
 *   h^[f,t] = sum_k tcoef[k][t] (W_k z_k)[f]             W_k = filt[cdm_group[u]][k], F x |P|
 * filt [2][nd][F][Pmax][2] with Pmax = (F + 1) / 2 (rows of group 1 zero-padded at odd F), tcoef
 * [nd][14][2], vconj [nd][nd][2]: f32 (re, im) device arrays; filt 8-byte aligned.  The products
 * W_k z_k run on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32).
 *
 * nrx_chest_lin: per DMRS symbol linear in frequency between the own pilots that bracket f -- beyond
 * the first / last pilot the line through the two nearest ones is extended -- then the same along
 * time between the DMRS symbols; a single pilot or a single DMRS symbol is repeated.  With f between
 * pilots p0 < p1 = p0 + 2, wf = (f - p0) / 2, and t between symbols t0 < t1, wt = (t - t0) / (t1 - t0):
 *   h^ = (1 - wt) ((1 - wf) x[p0,t0] + wf x[p1,t0]) + wt ((1 - wf) x[p0,t1] + wf x[p1,t1]).
 * filt / tcoef / vconj are not read.
 *
 * A NULL io / h_hat / active / h_out (nrx_chest_lmmse: or table), a filt that is not 8-byte
 * aligned, no <= 0, a DMRS symbol outside 0..13 or not ascending, or a cdm_group outside {0, 1} is
 * NRX_ERR_INVALID_ARG; T != 14, B outside 1..65535, U outside 1..16, F outside
 * 1..3300, A outside 1..16 or num_dmrs_symbols outside 1..4 is NRX_ERR_SHAPE.  Every argument is
 * checked before the first HIP call. */
typedef struct nrx_chest_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;   /* B, U (1..16), F (1..3300), T = 14 */
  int32_t num_rx_ant;          /* A, 1..16 */
  int32_t num_dmrs_symbols;    /* nd, 1..4 */
  int32_t dmrs_symbols[4];     /* ascending */
  int32_t cdm_group[16];       /* per port, 0/1 */
  double  no;                  /* noise variance per complex RE the estimate is made at, > 0 */
  const float* h_hat;          /* [B][U][F][T][2A], read at the own pilots only */
  const float* active;         /* [B][U] */
  const float* filt;           /* [2][nd][F][(F + 1) / 2][2] */
  const float* tcoef;          /* [nd][14][2] */
  const float* vconj;          /* [nd][nd][2] */
  float*       h_out;          /* [B][U][F][T][2A] */
} nrx_chest_io;

int nrx_chest_lmmse(const nrx_chest_io* io, void* stream);
int nrx_chest_lin(const nrx_chest_io* io, void* stream);

/* nrx_chest_lmmse3: the exact Wiener filter under the covariance R_s (x) R_t (x) R_f with white LS
 * noise sigma^2 = no / 2 -- the "s" stage of the reference's order "s-f-t" (utils/baseline_rx.py:
 * 160-195) included, for a generator with receive-antenna correlation.  It is diagonal in the three
 * eigenbases.  Host design, once per covariance (chest.lmmse3_design):
 *   R_s = V_s diag(mu) V_s^H (trace A),  R_t[D, D] = V_t diag(lambda) V_t^H (R_t of unit diagonal),
 *   R_f[P_g, P_g] = Q_g diag(nu_g) Q_g^H per CDM group g,  G_g = R_f[:, P_g] Q_g,
 *   tcoef[k][t] = (R_t[:, D] v_k)[t]   (not divided by lambda_k, unlike nrx_chest_lmmse's)
 * and per (b, u), g = cdm_group[u]:
 *   w[j,k,q] = sum_a conj(V_s[a][j]) sum_d conj(V_t[d][k]) sum_p conj(Q_g[p][q]) h_ls[a, P_p, D_d]
 *   c[j,k,q] = mu_j / (mu_j lambda_k nu_q + sigma^2) w[j,k,q]
 *   h^[a,f,t] = sum_j V_s[a][j] sum_k tcoef[k][t] sum_q G_g[f][q] c[j,k,q]
 * No eigenvalue is inverted, so nothing is dropped or ill-conditioned, and the tables do not depend
 * on no.  With R_s = I the estimate equals nrx_chest_lmmse's.  Tables, f32 device arrays with
 * Pmax = (F + 1) / 2, zero-padded where a group has fewer than Pmax pilots:
 *   qh [2][Pmax][Pmax][2]  rows of Q_g^H: qh[g][q][p] = conj(Q_g[p][q]);   gf [2][F][Pmax][2] = G_g
 *   nu [2][Pmax];  tcoef [nd][14][2];  vconj [nd][nd][2] = conj(v_k[d]);  lam [nd]
 *   vs [A][A][2] = V_s[a][j];  mu [A]
 * qh and gf 8-byte aligned.  Both matrix products run on the exact-f32 MFMA
 * (v_mfma_f32_16x16x4_f32); the workspace (nrx_chest3_workspace_size bytes, monotone in B) holds c,
 * rotated back to antennas, between the two kernels.  Guarantees and error codes are those of
 * nrx_chest_lmmse (every element of h_out written, zeros for inactive users and users without a
 * pilot, f32, no atomics, independent of the batch split, asynchronous on `stream`, every argument
 * checked before the first HIP call), and a NULL or not 4-byte aligned workspace or a NULL bytes is
 * NRX_ERR_INVALID_ARG, a workspace smaller than nrx_chest3_workspace_size NRX_ERR_WORKSPACE.
 * nrx_chest3_workspace_size reads only the shape fields. */
typedef struct nrx_chest3_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;   /* B, U (1..16), F (1..3300), T = 14 */
  int32_t num_rx_ant;          /* A, 1..16 */
  int32_t num_dmrs_symbols;    /* nd, 1..4 */
  int32_t dmrs_symbols[4];     /* ascending */
  int32_t cdm_group[16];       /* per port, 0/1 */
  double  no;                  /* noise variance per complex RE the estimate is made at, > 0 */
  const float* h_hat;          /* [B][U][F][T][2A], read at the own pilots only */
  const float* active;         /* [B][U] */
  const float* qh;             /* [2][Pmax][Pmax][2] */
  const float* gf;             /* [2][F][Pmax][2] */
  const float* nu;             /* [2][Pmax] */
  const float* tcoef;          /* [nd][14][2] */
  const float* vconj;          /* [nd][nd][2] */
  const float* lam;            /* [nd] */
  const float* vs;             /* [A][A][2] */
  const float* mu;             /* [A] */
  float*       h_out;          /* [B][U][F][T][2A] */
} nrx_chest3_io;

int nrx_chest3_workspace_size(const nrx_chest3_io* io, size_t* bytes);
int nrx_chest_lmmse3(const nrx_chest3_io* io, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- soft-output metrics
 * What a decoder would see of the LLRs, and how good a channel estimate is: the sums behind the
 * bitwise mutual information (BMI; Sionna's BitwiseMutualInformation, 1 - the binary cross-entropy
 * the reference trains on, neural_rx.py:687, in bits) and behind the NMSE of a channel estimate (the
 * reference's second loss, neural_rx.py:688).  The BMI is the rate a BICM decoder achieves with
 * exactly these LLRs; the coded BLER itself comes from the QC-LDPC decoder below.
 *
 * Contributing set: the one the error counters above count over -- (slot b, user u) with
 * active[b][u] > 0, symbols t whose bit is not set in dmrs_symbol_mask, every subcarrier f, bit
 * positions k < m with m = mcs_bits[mcs[b][u]] (MCS 0 when mcs == NULL; an index >= num_mcs is read as
 * num_mcs - 1); the head is mcs[b][u] when num_heads > 1, else 0.  LLR sign: L = log p(1)/p(0).  An LLR
 * equal to 0 in the set counts like any other: exclusion is by the masks, never by value.
 *
 * Loss of a contributing LLR L (f32) with sent bit c under scale s = scales[j]:
 *   z = (2c - 1) s L                         formed in float64
 *   loss_j = (max(-z, 0) + log1p(exp(-|z|))) / ln 2        bits
 * The unbounded linear term max(-z, 0) is computed and summed in float64, so the accuracy of a mean
 * does not depend on the size of the LLRs; the bounded term, in (0, ln 2], is the f32
 * log1pf(expf(.)) of the f32-rounded -|z|, summed in float64.  An LLR that is NaN or +-inf adds 1 to
 * nonfinite[u][mcs][k] and enters neither cnt nor any loss sum.
 *
 * Accumulators (device, owned and zeroed by the caller, only ever added to), M = num_mcs, S = num_scales:
 *   loss      f64 [U][M][8][S]     sum of loss_j over the contributing finite LLRs of (u, mcs, k)
 *   cnt       i64 [U][M][8]        their number
 *   nonfinite i64 [U][M][8]
 * On the host: bmi[m][k][j] = 1 - sum_u loss / sum_u cnt (it may be negative); the generalised mutual
 * information is its maximum over j (neural_rx_amd/softmetrics.py).
 *
 * Two launches: a work item is (slot, user, strip of at most NRX_SOFT_STRIP subcarriers) -- the
 * partition depends on the shape only -- and writes one partial record ([8][S] f64, two [8] i64) to the
 * workspace after a fixed-order reduction (across the wave, then across the waves); items of inactive
 * (slot, user) pairs exit after one load of active.  The second launch adds the partials of the active
 * items into the accumulators in ascending (b, strip) order, one thread per (u, k, j).  No atomics: the
 * same inputs give the same bits on every call.  No allocation, no host synchronisation; asynchronous on
 * `stream`, capturable into a hipGraph.  Every argument is checked before the first HIP call: a NULL io /
 * llr / bits / active / loss / cnt / nonfinite / workspace / bytes (mcs may be NULL), a workspace that is
 * not 8-byte aligned, num_scales outside 1..16, a scale that is not finite or <= 0, a bit width outside
 * 1..8 or a dmrs_symbol_mask outside 0..2^14 - 1 is NRX_ERR_INVALID_ARG; T != 14, B outside 1..65535,
 * F outside 1..3300, U outside 1..16, num_mcs outside 1..8, num_heads not in {1, num_mcs} or bits_stride <
 * max(mcs_bits) is NRX_ERR_SHAPE; a workspace smaller than nrx_llr_stats_workspace_size is
 * NRX_ERR_WORKSPACE. */
#define NRX_SOFT_STRIP 16
typedef struct nrx_llr_stats_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;   /* B (1..65535), U (1..16), F (1..3300), T = 14 */
  int32_t num_heads;           /* H heads in llr; head = mcs if H > 1 else 0 */
  int32_t bits_stride;         /* last dim of llr and bits */
  int32_t num_mcs;             /* M, 1..8 */
  int32_t mcs_bits[8];         /* 1..8 */
  int32_t dmrs_symbol_mask;
  int32_t num_scales;          /* S, 1..16 */
  int32_t pad_;
  double  scales[16];          /* each finite and > 0 */
  const float*   llr;          /* [H][B][U][F][T][bits_stride] (nrx_io.llr) */
  const uint8_t* bits;         /* [B][U][F][T][bits_stride] */
  const uint8_t* mcs;          /* [B][U] or NULL (= 0) */
  const float*   active;       /* [B][U] */
  double*  loss;               /* [U][M][8][S] accumulated */
  int64_t* cnt;                /* [U][M][8] accumulated */
  int64_t* nonfinite;          /* [U][M][8] accumulated */
} nrx_llr_stats_io;

int nrx_llr_stats_workspace_size(const nrx_llr_stats_io* io, size_t* bytes);
int nrx_llr_stats(const nrx_llr_stats_io* io, void* workspace, size_t workspace_bytes, void* stream);

/* Squared-error sums of a channel estimate h_est against the true channel h_true, both
 * [B][U][F][T][2A] f32 (nrx_gen_out.h_hat / .h layouts, nrx_io.h_ref): over the active (b, u), the
 * symbols whose bit is set in symbol_mask (0: all 14), every f and all 2A components,
 *   err[u] += sum (h_est - h_true)^2      (the difference formed in float64)
 *   ref[u] += sum h_true^2
 *   items[u] += 1 per active (b, u);      NMSE = sum_u err / sum_u ref.
 * The same two launches, partition, workspace discipline and determinism as nrx_llr_stats.  A NULL io /
 * h_est / h_true / active / err / ref / items / workspace / bytes, a workspace that is not 8-byte
 * aligned or a symbol_mask outside 0..2^14 - 1 is NRX_ERR_INVALID_ARG; T != 14, B outside 1..65535, F
 * outside 1..3300, U outside 1..16 or A outside 1..16 is NRX_ERR_SHAPE; a workspace smaller than
 * nrx_nmse_workspace_size is NRX_ERR_WORKSPACE. */
typedef struct nrx_nmse_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;   /* B, U (1..16), F (1..3300), T = 14 */
  int32_t num_rx_ant;          /* A, 1..16 */
  int32_t symbol_mask;         /* bit t set: symbol t is scored; 0 = all */
  const float* h_est;          /* [B][U][F][T][2A] */
  const float* h_true;         /* [B][U][F][T][2A] */
  const float* active;         /* [B][U] */
  double*  err;                /* [U] accumulated */
  double*  ref;                /* [U] accumulated */
  int64_t* items;              /* [U] accumulated */
} nrx_nmse_io;

int nrx_nmse_workspace_size(const nrx_nmse_io* io, size_t* bytes);
int nrx_chest_nmse(const nrx_nmse_io* io, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- QC-LDPC decoder
 * Layered belief propagation for a quasi-cyclic LDPC code, the decoder the reference puts behind
 * every receiver (TBDecoder: num_bp_iter = 20, cn_type = 'boxplus'; utils/neural_rx.py:1407-1413).
 * The code is data: a base matrix of circulant shifts that the caller passes.  The limits admit the
 * TS 38.212 base graphs, but the project ships and tests only codes it constructs itself
 * (neural_rx_amd/ldpc.py); a caller-supplied table goes through the same path.  Stated departures
 * from the reference: the project's own codes; no CRC, no segmentation and no bit interleaver; a
 * layered schedule where Sionna's is flooding.
 *
 * Code: shifts [mb][nb] int16 (host), -1 for no edge, else 0..z-1.  Block (i, j) with shift s
 * connects check i z + r to variable j z + (r + s) mod z, r = 0..z-1.  N = nb z.  Error counting
 * covers the information columns v < kb z.
 *
 * Decoding of one codeword from its channel LLRs l[v] = log p(0)/p(1) (positive: bit 0), in f32:
 *   init   APP[v] = clamp(l[v], +-llr_clip), a NaN input counts as 0; every check-to-variable
 *          message m_e = 0.
 *   One iteration is the layers i = 0..mb-1 in order.  In layer i every check r takes its edges
 *   e_0..e_{d-1} in ascending base-column order (2 <= d <= 32):
 *          t_k = APP[v_k] - m_k
 *          x_k = the extrinsic of the other edges' t (below)
 *          m_k <- clamp(x_k, +-llr_clip)
 *          APP[v_k] <- t_k + m_k
 *   Only the channel LLRs and the messages are clamped, never t or APP, so APP = l + sum of the
 *   variable's messages holds exactly and |APP| <= (1 + max column weight) llr_clip.
 *   boxplus (cn_type 0):  a [+] b = sgn(a) sgn(b) min(|a|, |b|) + (log1p(exp(-|a + b|)) - log1p(exp(-|a - b|)))
 *          with sgn(0) = 0; the correction is formed first, so a [+] b is exactly odd in a and in b and the
 *          decoder is exactly sign-symmetric.  P_0 = t_0, P_k = P_{k-1} [+] t_k (left fold); S_{d-1} = t_{d-1},
 *          S_k = S_{k+1} [+] t_k (right fold);  x_0 = S_1, x_{d-1} = P_{d-2}, else x_k = P_{k-1} [+] S_{k+1}.
 *   min-sum (cn_type 1):  x_k = ms_scale * (prod_{j != k} sgn(t_j) * min_{j != k} |t_j|) with sgn(0) = +1
 *          (the sign is the one of the comparison t < 0).
 *   After each iteration hard[v] = (APP[v] <= 0): a tie decides 1, so an all-erased input can never
 *   pass as the all-zero word.  parity_ok = every check of hard is satisfied.  With early_stop a
 *   codeword stops after the first iteration with parity_ok; iters = iterations run.  Without it
 *   iters = num_iter and parity_ok is the one after the last iteration.
 *   A codeword with skip[cw] != 0 is not decoded: its hard, app, iters and parity_ok are written 0.
 *
 * One launch runs all iterations: a workgroup owns 256 / z codewords (at least one), one thread per
 * check of a layer, APP in LDS, layers separated by a barrier; the messages live in LDS when they
 * fit next to APP, else in the workspace (nrx_ldpc_workspace_size, monotone in num_cw).  Early exit
 * is uniform over the workgroup.  No atomics: the same inputs give the same bits on every call,
 * independent of how the codewords are split into calls.  No allocation, no host synchronisation;
 * asynchronous on `stream`, capturable into a hipGraph.
 *
 * nrx_ldpc_create validates the host table before the first HIP call: a NULL code / shifts / out is
 * NRX_ERR_INVALID_ARG; mb outside 1..46, nb outside 2..68, nb <= mb, z outside 2..384 or kb outside
 * 1..nb-1 is NRX_ERR_SHAPE; a shift outside -1..z-1, a row weight outside 2..32 or an empty column
 * is NRX_ERR_INVALID_ARG.  device = -1 creates a handle without device tables: it answers
 * nrx_ldpc_workspace_size and runs every argument check of nrx_ldpc_decode, which then returns
 * NRX_ERR_INVALID_ARG ("no device").
 * nrx_ldpc_decode checks every argument before the first HIP call: a NULL io / llr_in / hard / iters
 * / parity_ok (app and skip may be NULL), num_iter outside 1..100, a cn_type other than 0 / 1,
 * an early_stop other than 0 / 1, cn_type 1 with ms_scale outside (0, 1], an llr_clip that is not
 * finite and > 0 is NRX_ERR_INVALID_ARG; num_cw outside 1..2^20 is NRX_ERR_SHAPE; then a NULL handle
 * or a NULL or not 16-byte aligned workspace is NRX_ERR_INVALID_ARG and a workspace smaller than
 * nrx_ldpc_workspace_size NRX_ERR_WORKSPACE. */
typedef struct nrx_ldpc_code {
  int32_t mb, nb, z, kb;       /* base rows 1..46, base columns 2..68 (> mb), lifting 2..384, 1 <= kb < nb */
  const int16_t* shifts;       /* host, [mb][nb] */
} nrx_ldpc_code;

typedef struct nrx_ldpc_io {
  int32_t num_cw;              /* 1..2^20 */
  int32_t num_iter;            /* 1..100 */
  int32_t cn_type;             /* 0 boxplus, 1 scaled min-sum */
  int32_t early_stop;          /* 0 / 1 */
  float   ms_scale;            /* cn_type 1: in (0, 1] */
  float   llr_clip;            /* > 0 */
  const float*   llr_in;       /* [num_cw][N], log p(0)/p(1) */
  const uint8_t* skip;         /* [num_cw] or NULL (= none) */
  uint8_t* hard;               /* [num_cw][N] */
  float*   app;                /* [num_cw][N] or NULL */
  int32_t* iters;              /* [num_cw] */
  uint8_t* parity_ok;          /* [num_cw] */
} nrx_ldpc_io;

typedef struct nrx_ldpc nrx_ldpc;

int nrx_ldpc_create(const nrx_ldpc_code* code, int32_t device, nrx_ldpc** out);
void nrx_ldpc_destroy(nrx_ldpc* h);
int nrx_ldpc_workspace_size(const nrx_ldpc* h, const nrx_ldpc_io* io, size_t* bytes);
int nrx_ldpc_decode(nrx_ldpc* h, const nrx_ldpc_io* io, void* workspace, size_t workspace_bytes, void* stream);

/* Slot glue of a coded evaluation.  The generator sends i.i.d. uniform bits c; they are read as the
 * all-zero codeword under the random scrambler c, so the descrambled LLR of a sent bit with engine
 * LLR L (Sionna sign, log p(1)/p(0)) is (2c - 1) L = log p(0)/p(1) towards the all-zero word.
 *
 * nrx_ldpc_gather writes llr_in [(b U + u) C + j][N] and skip [(b U + u) C + j] from the engine's LLR
 * tensor (contributing set, head and MCS rules of nrx_llr_stats).  Transmitted bit e of a (slot, user)
 * with m = mcs_bits[mcs[b][u]] is (i-th data RE in symbol-major order, bit k) with e = i m + k, the
 * order of nrx_llr_demap; n_data = F * (data symbols).  Codeword j takes e = j n_tx + e', e' in
 * [0, n_tx):   l[tx_col[e']] += (2c - 1) L   in f32, in ascending e', starting from col_prior[v]
 * (NULL: 0); repeats of a column accumulate, columns never listed stay at col_prior (puncturing and
 * shortening), an entry of tx_col outside 0..N-1 is dropped.  tx_col == NULL is the identity and
 * needs n_tx <= N.  A codeword is skipped (skip = 1, its row = col_prior) when the user is inactive
 * or j >= floor(n_data m / n_tx).  No floating-point atomics: the same bits on every call.
 * A NULL io / llr / bits / active / llr_in / skip, a bit width outside 1..8 or a dmrs_symbol_mask
 * outside 0..2^14 - 1 is NRX_ERR_INVALID_ARG; T != 14, B outside 1..65535, F outside 1..3300, U
 * outside 1..16, num_mcs outside 1..8, num_heads not in {1, num_mcs}, bits_stride < max(mcs_bits),
 * C outside 1..64, B U C > 2^20, N outside 4..26112, n_tx outside 1..2^20 or tx_col == NULL with
 * n_tx > N is NRX_ERR_SHAPE.  Checked before the first HIP call; asynchronous on `stream`. */
typedef struct nrx_ldpc_gather_io {
  int32_t batch, num_tx, num_subcarriers, num_symbols;   /* B (1..65535), U (1..16), F (1..3300), T = 14 */
  int32_t num_heads;           /* H heads in llr; head = mcs if H > 1 else 0 */
  int32_t bits_stride;         /* last dim of llr and bits */
  int32_t num_mcs;             /* 1..8 */
  int32_t mcs_bits[8];         /* 1..8 */
  int32_t dmrs_symbol_mask;
  int32_t num_cw_per_user;     /* C, 1..64 */
  int32_t n_tx;                /* transmitted bits per codeword */
  int32_t n;                   /* N */
  const float*   llr;          /* [H][B][U][F][T][bits_stride] (nrx_io.llr) */
  const uint8_t* bits;         /* [B][U][F][T][bits_stride] */
  const uint8_t* mcs;          /* [B][U] or NULL (= 0) */
  const float*   active;       /* [B][U] */
  const int32_t* tx_col;       /* device, [n_tx] or NULL (= identity) */
  const float*   col_prior;    /* device, [N] or NULL (= 0) */
  float*   llr_in;             /* [B U C][N] */
  uint8_t* skip;               /* [B U C] */
} nrx_ldpc_gather_io;

int nrx_ldpc_gather(const nrx_ldpc_gather_io* io, void* stream);

/* Coded error counters against the all-zero word, over the codewords with skip == 0:
 *   counts[u][0..3] += (information-bit errors, information bits, block errors, blocks)
 * where an information bit is a column v < num_info, a block is one (slot, user) with at least one
 * counted codeword, in error if any of them has hard != 0 in an information column.  counts has the
 * layout of nrx_count_errors (int64, device, accumulated), so the same all-reduce carries it.  With
 * iters and iter_counts both non-NULL, iter_counts[u][0..1] += (decoder iterations, codewords).
 * A NULL io / hard / skip / counts is NRX_ERR_INVALID_ARG; B outside 1..65535, U outside 1..16, C
 * outside 1..64, N outside 4..26112 or num_info outside 1..N is NRX_ERR_SHAPE. */
typedef struct nrx_ldpc_count_io {
  int32_t batch, num_tx;       /* B, U */
  int32_t num_cw_per_user;     /* C */
  int32_t n;                   /* N */
  int32_t num_info;            /* kb z */
  int32_t pad_;
  const uint8_t* hard;         /* [B U C][N] */
  const uint8_t* skip;         /* [B U C] */
  const int32_t* iters;        /* [B U C] or NULL */
  int64_t* counts;             /* [U][4] accumulated */
  int64_t* iter_counts;        /* [U][2] accumulated, or NULL */
} nrx_ldpc_count_io;

int nrx_ldpc_count(const nrx_ldpc_count_io* io, void* stream);

/* ---------------------------------------------------------------- training: loss, gradient, Adam
 * nrx_train_grad runs the CGNN of `desc` forward in f32 on the weights it is given, evaluates
 *   loss_data  = sum_r sum_m [ sum active[b,u] mcs_mask[b,u,m] l(z, bit) ] / (B U F (14 - n_dmrs) bits_m)
 *                l(z, bit) = max(z, 0) - bit z + log1p(exp(-|z|)) over the data symbols (those outside
 *                dmrs_symbol_mask) and the bits k < bits_m; LLR > 0 means bit 1, as in nrx_count_errors
 *   loss_chest = sum_r mean over [B,U,F,T,2A] of active[b,u] (h_ref - h)^2   (h_ref as the readout gives it and h
 *                as the generator gives it: the convention of nrx_chest_nmse, no rescaling by the slot norm)
 * over the readouts r (multiloss = 0: after iteration num_it; 1: after every iteration 1..num_it) and writes the
 * gradient of loss_data + w_chest loss_chest with respect to every weight.  With var_mcs_masking the one head is
 * sliced to bits_m for each m.  The per-slot input normalisation depends on no weight and has no backward.
 *
 * weights / grad: one flat f32 buffer each, the arrays of nrx_weight_layout(desc) concatenated in that order.
 * grad is overwritten; the arrays of iterations beyond num_it come back exactly zero.  loss = {loss_data,
 * loss_chest} (loss_chest = 0 when h is NULL).  llr / h_ref (optional): the last readout, in nrx_io's layouts.
 * All sums across workgroups are slab sums in a fixed order: the outputs are bit-reproducible from call to call.
 * Stateless, nothing allocated, no host synchronisation, everything on the caller's stream.
 *
 * Workspace: f32 activations kept position-major [P][C], P = B U F 14 positions (see csrc/nrx_train.hip for
 * the list); nrx_train_workspace_size gives the bytes.
 *
 * A NULL desc / io / y / pe / active / bits / weights / grad / loss / workspace / bytes, a NULL h_hat with
 * desc.use_h_hat, a NULL h with w_chest > 0, a float pointer that is not 4-byte aligned, a loss that is not
 * 8-byte aligned, a workspace that is not 256-byte aligned, num_it outside 1..desc.num_it, multiloss outside
 * 0/1, a dmrs_symbol_mask that is no mask of the 14 symbols or holds all of them, or a w_chest that is negative
 * or not finite is NRX_ERR_INVALID_ARG; T != 14, B / U / F outside nrx_forward's ranges, more than 2^24
 * positions or bits_stride < max(bits) is NRX_ERR_SHAPE; a topology nrx_create refuses is
 * NRX_ERR_UNSUPPORTED; a workspace smaller than nrx_train_workspace_size is NRX_ERR_WORKSPACE. */
typedef struct nrx_train_io {
  nrx_shape shape;
  int32_t num_it;              /* iterations to run, 1..desc.num_it */
  int32_t dmrs_symbol_mask;    /* bit t set: symbol t carries DMRS and no loss */
  int32_t multiloss;           /* 0: read out after the last iteration; 1: after every iteration */
  int32_t bits_stride;         /* bit axis of `bits`, >= max(desc.bits) */
  double w_chest;              /* weight of loss_chest in the gradient; 0 switches it off */
  const float* y;              /* as nrx_io */
  const float* pe;
  const float* h_hat;          /* may be NULL only if desc.use_h_hat == 0 */
  const float* active;
  const float* mcs_mask;       /* may be NULL: one-hot on MCS 0 */
  const uint8_t* bits;         /* [B][U][F][T][bits_stride], nrx_gen_out.bits */
  const float* h;              /* [B][U][F][T][2A] true channel, nrx_gen_out.h; may be NULL only if w_chest == 0 */
  const float* weights;        /* flat, Keras get_weights() order */
  float* grad;                 /* flat, like weights; overwritten */
  double* loss;                /* [2]: loss_data, loss_chest */
  float* llr;                  /* [H][B][U][F][T][bits_max] of the last readout, or NULL */
  float* h_ref;                /* [B][U][F][T][2A] of the last readout, or NULL */
} nrx_train_io;

int nrx_train_workspace_size(const nrx_desc* desc, const nrx_train_io* io, size_t* bytes);
int nrx_train_grad(const nrx_desc* desc, const nrx_train_io* io, void* workspace, size_t workspace_bytes,
                   void* stream);

/* One step's gradient from several calls: nrx_train_grad on a micro-batch of a step whose whole batch has
 * batch_total slots.  batch_total replaces shape.batch in every loss denominator,
 *   1 / (batch_total U F (14 - n_dmrs) bits_m)  for loss_data and  1 / (batch_total U F 14 2A)  for loss_chest,
 * and in their derivatives, so every term has the weight it has in the whole batch: the sum over micro-batches of
 * any sizes (equal or not) whose B add up to batch_total is the loss and the gradient of the whole batch, with
 * nothing to rescale afterwards.  accumulate = 0: grad and loss are overwritten, as nrx_train_grad does;
 * accumulate = 1: grad is not zeroed and every weight-gradient sum is added onto what it holds (in f64, rounded
 * once per sum), loss is added onto in f64.  The first call of a step overwrites, the others accumulate; the
 * launches and their order are those of nrx_train_grad, nothing is atomic, and a repeated sequence of calls gives
 * the same bits.  The arrays of iterations beyond num_it are written by no call: they stay exactly zero through a
 * sequence that starts with accumulate = 0.  llr / h_ref are those of the micro-batch of the call.
 * acc == NULL, accumulate = 0 with batch_total == shape.batch, and accumulate = 1 with batch_total == shape.batch
 * onto a zeroed grad and loss all give the bits of nrx_train_grad.  The workspace is that of
 * nrx_train_workspace_size for the call's own shape: a step needs the workspace of its largest micro-batch only.
 * accumulate outside 0/1 is NRX_ERR_INVALID_ARG; batch_total < shape.batch or > 65535 is NRX_ERR_SHAPE; the
 * other checks are those of nrx_train_grad, all before the first HIP call. */
typedef struct nrx_train_acc {
  int32_t accumulate;          /* 0: grad and loss are overwritten; 1: added onto what they hold */
  int32_t batch_total;         /* B of the whole step: replaces shape.batch in every loss denominator */
} nrx_train_acc;

int nrx_train_grad_acc(const nrx_desc* desc, const nrx_train_io* io, const nrx_train_acc* acc, void* workspace,
                       size_t workspace_bytes, void* stream);

/* One Adam step (Keras: tf.keras.optimizers.Adam, defaults 1e-3 / 0.9 / 0.999 / 1e-7) on n f32 elements, with
 * t = step:   m = b1 m + (1 - b1) g;   v = b2 v + (1 - b2) g^2;
 *             w -= lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)
 * The bias corrections are formed on the host in double; the update is one elementwise launch that works in
 * double on the stored (f32) m and v.  A NULL io / w / g / m / v or a pointer that is not 4-byte aligned, n < 0,
 * step < 1, lr / eps negative or not finite, or beta1 / beta2 outside [0, 1) is NRX_ERR_INVALID_ARG. */
typedef struct nrx_adam_io {
  int64_t n;
  float* w;
  const float* g;
  float* m;
  float* v;
  double lr, beta1, beta2, eps;
  int64_t step;                /* t >= 1 */
} nrx_adam_io;

int nrx_adam_step(const nrx_adam_io* io, void* stream);

/* Host helper: nearest-pilot positional encoding pe[U][F][T][2] for DMRS
 * configuration type 1 (restates onnx_utils.py:172-260 for the product path).
 * dmrs_symbols: the DMRS OFDM symbol indices; cdm_group[u] in {0,1}. */
int nrx_compute_pe(int32_t num_tx, int32_t num_subcarriers, int32_t num_symbols,
                   const int32_t* dmrs_symbols, int32_t num_dmrs_symbols,
                   const int32_t* cdm_group, float* pe_out);

/* Algorithmic FLOPs of one forward per resource element per user
 * (SURVEY.md 8(d) formula). */
double nrx_flops_per_re_user(const nrx_desc* desc, int32_t num_it);

/* Per-kernel timing.  While enabled, nrx_forward records a HIP event pair around
 * every kernel launch on the launch stream (not graph-capture safe).  Kernel ids:
 * 0 norm, 1 state-init (+ fused aggregation tail), 2 state-update (+ fused aggregation
 * or readout tail), 3 the one-launch forward (StateInit + updates + readouts; see
 * nrx_fused_status for when it is taken), 4 the register-resident state-update launch
 * (nrx_update_schedule), 5 the leave-one-out combine pass of U > 2 users (k_combine: after
 * StateInit and after every aggregation update), 6 the whole-column state-update launch, 7 the
 * whole-column StateInit launch (nrx_update_schedule).
 * nrx_profile_enable(h, 1) (re)starts the counters; nrx_profile_read waits for the
 * recorded events and returns the launch count and summed device time of a kernel. */
int nrx_profile_enable(nrx_handle* h, int32_t enable);
int nrx_profile_read(nrx_handle* h, int32_t kernel, int64_t* launches, double* total_ms);

/* The one-launch forward (k_forward, f16 only): StateInit, every update and the readouts as ONE
 * persistent launch whose items wait on per-(stage, slot) counters in a handle-owned buffer.
 * It applies to f16 forwards with 24-row strips and at least two items per CU, U <= 8 users,
 * 2A <= 32 (16 rx antennas), Var-IO (one StateInit stage per MCS), up to 8 iterations
 * (num_init + num_it <= 12) and up to three LLR heads.  Which shapes take it by default is set
 * by nrx_fused_config (default: the shapes where it measured faster -- U <= 2 with at least four
 * stages, i.e. Var-IO and 8-iteration models such as BASELINE cfg4 / cfg4'; the 2-iteration
 * bench forward, U > 2 and the large grids run the three-launch path).  status[3] since the
 * last reset: [0] error bits (1: a bounded dependency wait timed out, 2: items left undone --
 * the results of that forward are invalid), [1] update items whose inputs were not complete
 * when the previous item polled for them, [2] the polls those waits took.  Blocking: waits for
 * an event the handle recorded behind its last one-launch forward (not for the caller's stream,
 * which may have been destroyed since); reset != 0 clears them.  Returns NRX_ERR_FUSED (message
 * with the bits) when the error word is non-zero, so a caller that only checks the status code
 * cannot miss it; status[] is filled either way.
 * Forwards on one handle must not run concurrently on several streams (the counters are per
 * handle): nrx_forward / nrx_forward_ex / nrx_forward_aerial return NRX_ERR_BUSY, before
 * launching anything, when a forward that would take this path arrives on a stream other than
 * the previous one-launch forward's while that forward has not finished.  Forwards captured
 * into a hipGraph record no event: graph replays are outside this guard, so a caller replays
 * one handle's graphs on one stream.  NRX_FUSED in the environment (read by nrx_create): 0/off
 * the three-launch path, 1/on the default, 2/force wherever the path applies; any other value
 * fails nrx_create with NRX_ERR_INVALID_ARG. */
int nrx_fused_status(nrx_handle* h, int32_t* status, int32_t reset);

/* Per-handle control of the one-launch forward: enable = 0 no one-launch forward of any kind
 * (k_forward or k_fwd_col); 1 (default) k_forward only for the shapes it applies to by default
 * (U <= 2 with conv1 reading its rows from memory, at least four stages) that the column launches
 * do not take -- no BASELINE shape since round 6; 2 k_forward for every shape it applies to
 * (also the 2-iteration bench forward, U <= 8 and 2A <= 32 with staged z images; outputs
 * identical to the launch loop); > 2 invalid.  The initial value comes from NRX_FUSED at
 * nrx_create; spin_limit = dependency-wait polls before the timeout error (0: the default,
 * ~0.5 s); inject_err = error bits the next forwards set in the error word (test hook: callers
 * must surface them; 0: none).  Any argument < 0 leaves that setting unchanged. */
int nrx_fused_config(nrx_handle* h, int32_t enable, int32_t spin_limit, int32_t inject_err);

/* Stage schedule of the three-launch f16 forward, a mask (24-row strip tier):
 *   bit 0 (1)  the aggregation update stages (every iteration but the last) and
 *   bit 1 (2)  the readout update stage (the last) as the register-resident 16-row launch
 *              (k_update_rr: layer outputs kept in registers, weights staged once per workgroup);
 *   bit 2 (4)  the aggregation update stages and
 *   bit 3 (8)  the readout update stage as the whole-column launch (k_update_col: 48-position
 *              items, 6 register-resident rows per wave, no halo on grids of <= 48 subcarriers;
 *              taken over bits 0 / 1);
 *   bit 4 (16) StateInit as the whole-column launch (k_init_col: one StateInit, 2A = 8);
 *   bit 5 (32) the one-launch column forward (k_fwd_col: StateInit + every update in one
 *              persistent launch, at most one item per CU and stage; opt-in, measured slower);
 *   bit 6 (64) the column updates on grids wider than one column too (44-output strips;
 *              measured slower than the RR launch there, so off by default).
 * Each applies where it can -- the update launches with conv1 reading its rows from memory (any
 * U: for U > 2 the combine pass's a_u planes), 2A <= 32, for the readout stage one LLR head
 * whose readout fits -- the strip kernels elsewhere.  0: the strip kernels everywhere; < 0
 * unchanged; > 127 invalid.  Outputs are bit-identical either way.  The initial value comes from
 * NRX_UPDATE_RR (0..127) at nrx_create; the default (29: column StateInit and column updates on
 * single-column grids, the RR aggregation update elsewhere) is the mask measured fastest on every
 * BASELINE shape.  Kernel ids 6 / 7 / 8 of nrx_profile_read time the column
 * update / StateInit / one-launch column forward. */
int nrx_update_schedule(nrx_handle* h, int32_t update_rr);

const char* nrx_last_error(void);
int32_t nrx_api_version(void);
/* Content hash of the sources this library was built from (16 hex digits; set at link time by
 * neural_rx_amd/build.py).  Recorded with every committed counter capture so that a bench line
 * can tell whether the counters it quotes were taken from the library that is running. */
const char* nrx_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* NRX_H_ */
