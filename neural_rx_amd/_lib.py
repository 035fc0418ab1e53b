"""ctypes binding of ``libnrx.so`` (the C ABI declared in ``include/nrx.h``).

There is deliberately no fallback: if the HIP library is missing or fails to load,
every engine entry point raises ``NRXLibraryError``.  Build it with
``python -m neural_rx_amd.build`` (or ``__graft_entry__.build()``).

The ABI is stated once each way: the ``Structure`` classes (built from the field runs the
descriptors share; tests/test_abi_layout.py holds every size and offset against the header) and
``SIGNATURES``, which ``load()`` applies and ``EXPORTS`` lists (tests/test_abi.py holds it against
the header).  What the wrappers do with them is in ``_call.py``.
"""
from __future__ import annotations

import ctypes
import os

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
# NRX_LIB_PATH: diagnostic override (kernel-variant A/B runs); the default is the in-tree build
LIB_PATH = os.environ.get("NRX_LIB_PATH") or os.path.join(LIB_DIR, "libnrx.so")

NRX_OK = 0
NRX_ERR_INVALID_ARG = -1
NRX_ERR_WORKSPACE = -6
NRX_ERR_BUSY = -7
NRX_ERR_FUSED = -8
NRX_PREC_F16 = 0
NRX_PREC_F32X = 1
PRECISIONS = {"f16": NRX_PREC_F16, "fp16": NRX_PREC_F16, "f32x": NRX_PREC_F32X,
              "parity": NRX_PREC_F32X}

# nrx_cfo_io.ref_mode (NRX_CFO_REF_*)
CFO_REF_NEAREST_DMRS = 0
CFO_REF_ZERO = 1
# nrx_ofdm_io.precision / grid_layout (NRX_OFDM_*)
OFDM_PRECISIONS = {"f32": 0, "f64": 1}
OFDM_LAYOUTS = {"planar": 0, "cgnn": 1}
# enum nrx_y_layout
Y_LAYOUTS = {"cgnn": 0, "sionna": 1, "split": 2}
KERNELS = ["norm", "state_init", "state_update", "forward", "state_update_rr", "combine", "state_update_col",
           "state_init_col", "forward_col"]


class NRXLibraryError(RuntimeError):
    pass


class NRXError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"nrx error {code}: {msg}")
        self.code = code


I32, F64, PTR = ctypes.c_int32, ctypes.c_double, ctypes.c_void_p


def _i32(*names):
    return [(n, I32) for n in names]


def _f64(*names):
    return [(n, F64) for n in names]


def _ptr(*names):
    return [(n, PTR) for n in names]


# The field runs the descriptors of include/nrx.h share, under the same names everywhere (which is what lets
# _call.fill_grid / fill_mcs / fill_dmrs take any of them): the grid, the grid with its antennas, the MCS
# block, the DMRS block and the cover codes.
GRID = _i32("batch", "num_tx", "num_subcarriers", "num_symbols")
GRID_ANT = GRID + _i32("num_rx_ant")
MCS = _i32("bits_stride", "num_mcs") + [("mcs_bits", I32 * 8)] + _i32("dmrs_symbol_mask")
DMRS = _i32("num_dmrs_symbols") + [("dmrs_symbols", I32 * 4), ("cdm_group", I32 * 16)]
COVERS = [("focc", I32 * 16), ("tocc", I32 * 16)] + _i32("despread_f", "despread_t")


class nrx_desc(ctypes.Structure):
    _fields_ = (_i32("num_rx_ant", "d_s", "num_it", "num_mcs") + [("bits", I32 * 8)] + _i32("var_mcs_masking")
                + [("init_units", I32 * 2)] + _i32("agg_units") + [("state_units", I32 * 2)]
                + _i32("readout_units", "use_h_hat"))


class nrx_shape(ctypes.Structure):
    _fields_ = GRID


class nrx_io(ctypes.Structure):
    _fields_ = ([("shape", nrx_shape)] + _i32("num_it", "precision")
                + _ptr("y", "pe", "h_hat", "active", "mcs_mask", "llr", "h_ref"))


class nrx_aerial_io(ctypes.Structure):
    _fields_ = ([("shape", nrx_shape)] + _i32("num_it", "precision", "num_dmrs_symbols", "num_dmrs_subcarriers")
                + _ptr("y_real", "y_imag", "h_ls_real", "h_ls_imag", "dmrs_port_mask", "dmrs_ofdm_pos",
                       "dmrs_subcarrier_pos", "llr", "h_hat"))


class nrx_gen_desc(ctypes.Structure):
    _fields_ = (GRID_ANT + _i32("num_dmrs_symbols") + [("dmrs_symbols", I32 * 4)] + _i32("dmrs_symbol_mask")
                + [("cdm_group", I32 * 16)] + _i32("num_mcs") + [("mcs_bits", I32 * 8), ("mcs_of_user", I32 * 16)]
                + _i32("num_active", "num_taps", "num_sinusoids", "pad_")
                + _f64("max_delay_s", "max_doppler_hz", "subcarrier_spacing", "no")
                + [("seed", ctypes.c_uint64), ("slot_offset", ctypes.c_int64)])


class nrx_gen_out(ctypes.Structure):
    _fields_ = (_ptr("y", "h_hat", "h", "active", "mcs_mask", "mcs", "bits") + _i32("bits_stride", "pad_")
                + _ptr("y_real", "y_imag", "h_ls_real", "h_ls_imag"))


class nrx_gen_chan(ctypes.Structure):
    _fields_ = [("max_delay_s", F64 * 16), ("max_doppler_hz", F64 * 16)] + _ptr("rx_mix")


class nrx_gen_cfo(ctypes.Structure):
    _fields_ = [("cfo_hz", F64 * 16)] + _i32("constant", "fft_size", "h_with_phase", "pad_") + _ptr("eps_out")


class nrx_cfo_io(ctypes.Structure):
    _fields_ = GRID_ANT + DMRS + _i32("ref_mode", "sign") + _ptr("h_in", "active", "eps", "h_out")


class nrx_ls_io(ctypes.Structure):
    _fields_ = GRID_ANT + DMRS + COVERS + _ptr("y", "pilots", "active", "h_hat", "h_ls_real", "h_ls_imag")


class nrx_gen_dmrs(ctypes.Structure):
    _fields_ = COVERS + _ptr("pilots_out")


class nrx_gen_cir(ctypes.Structure):
    _fields_ = (_i32("num_examples", "num_paths", "num_time_steps", "select", "normalize", "pad_") + _f64("f_offset")
                + _ptr("a", "tau", "index"))


class nrx_ofdm_io(ctypes.Structure):
    _fields_ = (_i32("batch", "num_streams", "grid_subcarriers", "num_symbols", "fft_size", "first_bin")
                + [("cp_length", I32 * 14)] + _i32("precision", "grid_layout", "timing_advance")
                + [("offset", I32 * 16), ("num_samples", ctypes.c_int64)] + _f64("pa_asat", "pa_smoothness")
                + _ptr("grid", "samples"))


class nrx_gen_td(ctypes.Structure):
    _fields_ = (_i32("fft_size", "first_bin") + [("cp_length", I32 * 14), ("delay", I32 * 16)]
                + _i32("pa_enable", "h_with_delay") + _f64("pa_ibo_db", "pa_smoothness") + _ptr("x_out"))


class nrx_tc_io(ctypes.Structure):
    _fields_ = (_i32("batch", "num_tx", "num_rx_ant", "num_paths", "num_sinusoids", "l_min", "l_max", "pad_")
                + [("num_samples", ctypes.c_int64), ("n0", ctypes.c_int64)] + _f64("sample_rate")
                + _ptr("tau", "g0", "fd", "x", "rx_mix", "r"))


class nrx_gen_tc(ctypes.Structure):
    _fields_ = (_i32("fft_size", "first_bin") + [("cp_length", I32 * 14)]
                + _i32("l_min", "l_max", "timing_advance", "pad_") + _ptr("r_out", "x_out"))


class nrx_gen_noise(ctypes.Structure):
    _fields_ = _ptr("no_slot")


class nrx_count_io(ctypes.Structure):
    _fields_ = GRID + _i32("num_heads") + MCS + _ptr("llr", "bits", "mcs", "active", "counts")


class nrx_lmmse_io(ctypes.Structure):
    _fields_ = GRID_ANT + MCS + _i32("pad_") + _f64("no", "err_var") + _ptr("y", "h", "active", "mcs", "llr")


class nrx_kbest_io(ctypes.Structure):
    _fields_ = (GRID_ANT + MCS + _i32("k") + _f64("no", "err_var", "llr_clip")
                + _ptr("y", "h", "active", "mcs", "llr"))


class nrx_cov_io(ctypes.Structure):
    _fields_ = GRID_ANT + _i32("pad_") + _ptr("h", "acc")


class nrx_cov_space_io(ctypes.Structure):
    _fields_ = nrx_cov_io._fields_


class nrx_chest_io(ctypes.Structure):
    _fields_ = GRID_ANT + DMRS + _f64("no") + _ptr("h_hat", "active", "filt", "tcoef", "vconj", "h_out")


class nrx_chest3_io(ctypes.Structure):
    _fields_ = (GRID_ANT + DMRS + _f64("no")
                + _ptr("h_hat", "active", "qh", "gf", "nu", "tcoef", "vconj", "lam", "vs", "mu", "h_out"))


class nrx_llr_stats_io(ctypes.Structure):
    _fields_ = (GRID + _i32("num_heads") + MCS + _i32("num_scales", "pad_") + [("scales", F64 * 16)]
                + _ptr("llr", "bits", "mcs", "active", "loss", "cnt", "nonfinite"))


class nrx_nmse_io(ctypes.Structure):
    _fields_ = GRID_ANT + _i32("symbol_mask") + _ptr("h_est", "h_true", "active", "err", "ref", "items")


class nrx_ldpc_code(ctypes.Structure):
    _fields_ = _i32("mb", "nb", "z", "kb") + _ptr("shifts")


class nrx_ldpc_io(ctypes.Structure):
    _fields_ = (_i32("num_cw", "num_iter", "cn_type", "early_stop")
                + [("ms_scale", ctypes.c_float), ("llr_clip", ctypes.c_float)]
                + _ptr("llr_in", "skip", "hard", "app", "iters", "parity_ok"))


class nrx_ldpc_gather_io(ctypes.Structure):
    _fields_ = (GRID + _i32("num_heads") + MCS + _i32("num_cw_per_user", "n_tx", "n")
                + _ptr("llr", "bits", "mcs", "active", "tx_col", "col_prior", "llr_in", "skip"))


class nrx_ldpc_count_io(ctypes.Structure):
    _fields_ = (_i32("batch", "num_tx", "num_cw_per_user", "n", "num_info", "pad_")
                + _ptr("hard", "skip", "iters", "counts", "iter_counts"))


class nrx_train_io(ctypes.Structure):
    _fields_ = ([("shape", nrx_shape)] + _i32("num_it", "dmrs_symbol_mask", "multiloss", "bits_stride") + _f64("w_chest")
                + _ptr("y", "pe", "h_hat", "active", "mcs_mask", "bits", "h", "weights", "grad", "loss", "llr", "h_ref"))


class nrx_train_acc(ctypes.Structure):
    _fields_ = _i32("accumulate", "batch_total")


class nrx_adam_io(ctypes.Structure):
    _fields_ = ([("n", ctypes.c_int64)] + _ptr("w", "g", "m", "v") + _f64("lr", "beta1", "beta2", "eps")
                + [("step", ctypes.c_int64)])


def _signatures():
    c = ctypes
    P = c.POINTER
    RC, I, V, Z, PZ = c.c_int, c.c_int32, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t)
    desc, gen, chan, cfo, dmrs, cir, out = (P(nrx_desc), P(nrx_gen_desc), P(nrx_gen_chan), P(nrx_gen_cfo),
                                            P(nrx_gen_dmrs), P(nrx_gen_cir), P(nrx_gen_out))
    td, tc = P(nrx_gen_td), P(nrx_gen_tc)
    run = [V, Z, V]          # workspace, workspace_bytes, stream
    return {
        "nrx_create": (RC, [desc, P(V), P(c.c_int64), I, I, P(V)]),
        "nrx_weight_layout": (RC, [desc, P(I), P(c.c_int64), I]),
        "nrx_workspace_size": (RC, [V, P(nrx_shape), I, PZ]),
        "nrx_forward": (RC, [V, P(nrx_io)] + run),
        "nrx_workspace_size_ex": (RC, [V, P(nrx_shape), I, I, PZ]),
        "nrx_forward_ex": (RC, [V, P(nrx_io), I, V] + run),
        "nrx_destroy": (None, [V]),
        "nrx_compute_pe": (RC, [I, I, I, P(I), I, P(I), P(c.c_float)]),
        "nrx_flops_per_re_user": (c.c_double, [desc, I]),
        "nrx_last_error": (c.c_char_p, []),
        "nrx_api_version": (I, []),
        "nrx_build_id": (c.c_char_p, []),
        "nrx_profile_enable": (RC, [V, I]),
        "nrx_profile_read": (RC, [V, I, P(c.c_int64), P(c.c_double)]),
        "nrx_fused_status": (RC, [V, V, I]),
        "nrx_fused_config": (RC, [V, I, I, I]),
        "nrx_update_schedule": (RC, [V, I]),
        "nrx_aerial_workspace_size": (RC, [V, P(nrx_aerial_io), PZ]),
        "nrx_forward_aerial": (RC, [V, P(nrx_aerial_io)] + run),
        "nrx_aerial_preprocess": (RC, [V, P(nrx_aerial_io), V, V, V, V, V]),
        "nrx_llr_demap": (RC, [V, I, I, I, I, I, I, V, I, V, V]),
        "nrx_gen_workspace_size": (RC, [gen, PZ]),
        "nrx_generate_slots": (RC, [gen, out] + run),
        "nrx_generate_slots_ex": (RC, [gen, chan, out] + run),
        "nrx_gen_workspace_size_cfo": (RC, [gen, cfo, PZ]),
        "nrx_generate_slots_cfo": (RC, [gen, chan, cfo, out] + run),
        "nrx_gen_workspace_size_dmrs": (RC, [gen, cfo, dmrs, PZ]),
        "nrx_generate_slots_dmrs": (RC, [gen, chan, cfo, dmrs, out] + run),
        "nrx_gen_workspace_size_cir": (RC, [gen, cfo, dmrs, cir, PZ]),
        "nrx_generate_slots_cir": (RC, [gen, chan, cfo, dmrs, cir, out] + run),
        "nrx_generate_taps": (RC, [gen, chan, V, V] + run),
        "nrx_ofdm_modulate": (RC, [P(nrx_ofdm_io), V]),
        "nrx_ofdm_demodulate": (RC, [P(nrx_ofdm_io), V]),
        "nrx_gen_workspace_size_td": (RC, [gen, cfo, dmrs, cir, td, PZ]),
        "nrx_generate_slots_td": (RC, [gen, chan, cfo, dmrs, cir, td, out] + run),
        "nrx_time_channel": (RC, [P(nrx_tc_io), V]),
        "nrx_gen_workspace_size_tc": (RC, [gen, chan, cfo, dmrs, cir, td, tc, PZ]),
        "nrx_generate_slots_tc": (RC, [gen, chan, cfo, dmrs, cir, td, tc, out] + run),
        "nrx_generate_slots_no": (RC, [gen, chan, cfo, dmrs, cir, td, tc, P(nrx_gen_noise), out] + run),
        "nrx_count_errors": (RC, [P(nrx_count_io), V]),
        "nrx_cfo_estimate": (RC, [P(nrx_cfo_io), V]),
        "nrx_cfo_rotate": (RC, [P(nrx_cfo_io), V]),
        "nrx_ls_estimate": (RC, [P(nrx_ls_io), V]),
        "nrx_lmmse_detect": (RC, [P(nrx_lmmse_io), V]),
        "nrx_kbest_workspace_size": (RC, [P(nrx_kbest_io), PZ]),
        "nrx_kbest_detect": (RC, [P(nrx_kbest_io)] + run),
        "nrx_cov_workspace_size": (RC, [P(nrx_cov_io), PZ]),
        "nrx_cov_accumulate": (RC, [P(nrx_cov_io)] + run),
        "nrx_cov_space_workspace_size": (RC, [P(nrx_cov_space_io), PZ]),
        "nrx_cov_space_accumulate": (RC, [P(nrx_cov_space_io)] + run),
        "nrx_chest_lmmse": (RC, [P(nrx_chest_io), V]),
        "nrx_chest_lin": (RC, [P(nrx_chest_io), V]),
        "nrx_chest3_workspace_size": (RC, [P(nrx_chest3_io), PZ]),
        "nrx_chest_lmmse3": (RC, [P(nrx_chest3_io)] + run),
        "nrx_llr_stats_workspace_size": (RC, [P(nrx_llr_stats_io), PZ]),
        "nrx_llr_stats": (RC, [P(nrx_llr_stats_io)] + run),
        "nrx_nmse_workspace_size": (RC, [P(nrx_nmse_io), PZ]),
        "nrx_chest_nmse": (RC, [P(nrx_nmse_io)] + run),
        "nrx_ldpc_create": (RC, [P(nrx_ldpc_code), I, P(V)]),
        "nrx_ldpc_destroy": (None, [V]),
        "nrx_ldpc_workspace_size": (RC, [V, P(nrx_ldpc_io), PZ]),
        "nrx_ldpc_decode": (RC, [V, P(nrx_ldpc_io)] + run),
        "nrx_ldpc_gather": (RC, [P(nrx_ldpc_gather_io), V]),
        "nrx_ldpc_count": (RC, [P(nrx_ldpc_count_io), V]),
        "nrx_train_workspace_size": (RC, [desc, P(nrx_train_io), PZ]),
        "nrx_train_grad": (RC, [desc, P(nrx_train_io)] + run),
        "nrx_train_grad_acc": (RC, [desc, P(nrx_train_io), P(nrx_train_acc)] + run),
        "nrx_adam_step": (RC, [P(nrx_adam_io), V]),
    }


# {export: (restype, argtypes)}: every symbol of include/nrx.h (checked by tests/test_abi.py)
SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)

# subcarriers per work item of nrx_llr_stats / nrx_chest_nmse (NRX_SOFT_STRIP of include/nrx.h)
SOFT_STRIP = 16

_lib = None


def load(path: str = LIB_PATH):
    """Load libnrx.so once; raise NRXLibraryError if it is missing or broken."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NRXLibraryError(
            f"{path} not found: the MI355X engine is not built "
            "(run `python -m neural_rx_amd.build`); there is no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7.  Load
    # torch first so that libnrx's DT_NEEDED libamdhip64.so.7 binds to that copy
    # (by soname) instead of pulling /opt/rocm's as a second runtime.
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover - plain C users
        pass
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover - depends on the box
        raise NRXLibraryError(f"failed to load {path}: {e}") from e
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc: int):
    if rc != NRX_OK:
        msg = _lib.nrx_last_error().decode() if _lib is not None else "?"
        raise NRXError(rc, msg)


def make_desc(spec) -> nrx_desc:
    d = nrx_desc()
    d.num_rx_ant = spec.num_rx_ant
    d.d_s = spec.d_s
    d.num_it = spec.num_it
    d.num_mcs = spec.num_mcs
    for i, b in enumerate(spec.bits):
        d.bits[i] = b
    d.var_mcs_masking = int(spec.masking)
    d.init_units[0], d.init_units[1] = spec.init_units
    d.agg_units = spec.agg_units
    d.state_units[0], d.state_units[1] = spec.state_units
    d.readout_units = spec.readout_units
    d.use_h_hat = int(spec.use_h_hat)
    return d
