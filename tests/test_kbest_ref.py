"""The numpy K-best reference (tests/kbest_ref.py) and the host side of ``nrx_kbest_detect``;
no GPU.

The detector is defined by this project, so the reference is pinned by what it must equal: the
exhaustive max-log ML detector where 64 survivors hold every leaf (K1, K2), the clipped LMMSE
detector at one user (K1; ties the sign and bit-to-axis conventions to the existing baseline), and
its bit-error counts on the oracle generator's slots (tests/kbest_ref.CASES).  The conditions the
GPU gates of tests/test_gpu_kbest.py rest on are asserted here on the reference alone.  The
argument checks of the library run before its first HIP call, so their status codes are checked
here through the real ``libnrx.so``.

Figures of the reference on the oracle generator's slots (floor = max |r32 - r64| / max(1, |r64|)):

    case  floor    min pivot ratio  share |llr| = clip  K-best / LMMSE bit errors
    K3    2.9e-5   2.1e-2           0.29                156 / 457 of 6912
    K4    1.4e-5   0.39             0.44                 66 /  90 of 5184
    K5    4.8e-6   6.7e-3           0.13                107 / 335 of 4608
    K6    5.3e-6   0.89             0.37                103 / 116 of 4032   (0 dB; 0.998 on the clip at 12 dB)
"""
import ctypes
import functools

import numpy as np
import pytest

from neural_rx_amd import _lib
from oracle import synth_ref as S

from tests import kbest_ref as K
from tests import lmmse_ref as R

OK, INVALID_ARG, SHAPE, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3, -6


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, slots, f64 LLRs, min pivot ratio) of a case with perfect CSI, computed once"""
    spec = K.case_spec(name)
    g = S.generate(spec)
    llr, ratio = K.kbest_detect(*_args(spec, g), return_pivot=True)
    llr.setflags(write=False)
    return spec, g, llr, ratio


def _args(spec, g):
    return g.y, g.h, g.active, g.mcs, spec.mcs_bits, spec.no, spec.dmrs_symbols


@pytest.mark.parametrize("name", ["K1", "K2"])
def test_exhaustive_cases_equal_max_log_ml(name):
    spec, g, llr, _ = _case(name)
    ml = K.ml_detect(*_args(spec, g))
    e = float(np.abs(llr - ml).max())
    print(f"{name}: max |kbest - ml| {e:.1e}")
    assert e <= 1e-9
    assert np.abs(ml).max() == 20.0 and (np.abs(ml) < 20.0).any()


def test_one_user_equals_clipped_lmmse():
    spec, g, llr, _ = _case("K1")
    lm = np.clip(R.lmmse_detect(*_args(spec, g)), -20.0, 20.0)
    e = float(np.abs(llr - lm).max())
    print(f"K1: max |kbest - clip(lmmse)| {e:.1e}")
    assert e <= 1e-9


@pytest.mark.parametrize("name", K.PRUNED)
def test_conditions_of_the_gpu_gates(name):
    spec, g, llr, ratio = _case(name)
    r32 = K.kbest_detect(*_args(spec, g), dtype=np.float32)
    assert r32.dtype == np.float32
    floor = float(np.max(np.abs(r32 - llr) / np.maximum(1.0, np.abs(llr))))
    used = llr != 0
    share = float((np.abs(llr[used]) == 20.0).mean())
    print(f"{name}: floor {floor:.1e}  min pivot ratio {ratio:.1e}  share on the clip {share:.2f}")
    assert floor <= 1e-4
    assert ratio >= 1e-3
    assert share < 0.5


@pytest.mark.parametrize("name", list(K.CASES))
def test_reference_counts(name):
    spec, g, llr, _ = _case(name)
    kb = S.count_errors(llr, g.bits, g.mcs, spec.mcs_bits, g.active, spec.dmrs_symbols).sum(0)
    lm = S.count_errors(R.lmmse_detect(*_args(spec, g)), g.bits, g.mcs, spec.mcs_bits, g.active,
                        spec.dmrs_symbols).sum(0)
    assert (int(kb[0]), int(lm[0]), int(kb[1])) == K.CASES[name][10] and kb[1] == lm[1]
    if name in ("K3", "K5"):
        assert kb[0] < lm[0]


def test_table_of_the_issue():
    assert K.CASES["K3"][10] == (156, 457, 6912) and K.CASES["K5"][10] == (107, 335, 4608)


def test_zeros_for_inactive_dmrs_and_unused_bits():
    spec, g, llr, _ = _case("K6")
    llr = llr[0]
    assert (g.active == 0).any() and len(np.unique(g.mcs[g.active > 0])) > 1
    assert np.all(llr[g.active == 0] == 0)
    assert np.all(llr[:, :, :, list(spec.dmrs_symbols)] == 0)
    data = [t for t in range(14) if t not in spec.dmrs_symbols]
    for b, u in zip(*np.nonzero(g.active)):
        m = spec.mcs_bits[g.mcs[b, u]]
        assert np.all(llr[b, u][..., m:] == 0)
        assert np.all(llr[b, u][:, data, :m] != 0)


def test_all_zero_channel_gives_zero_llrs():
    y = np.ones((1, 3, 14, 8), np.float32)
    llr = K.kbest_detect(y, np.zeros((1, 2, 3, 14, 8), np.float32), np.ones((1, 2), np.float32), None, (4,), 0.1, (2,))
    assert np.all(llr == 0)


def test_smaller_k_is_a_subset_search():
    """k = 1 is decision feedback: one path, so every LLR of a used element sits on the clip"""
    spec, g, _, _ = _case("K3")
    one = K.kbest_detect(*_args(spec, g), k=1)
    assert set(np.unique(np.abs(one))) == {0.0, 20.0}


# ---- the library's argument checks (host only) ----------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def _io(**kw):
    """A valid descriptor whose pointers are non-null but never dereferenced on the host: every
    case below must be rejected before the first HIP call."""
    io = _lib.nrx_kbest_io()
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = 2, 2, 12, 14
    io.num_rx_ant, io.bits_stride, io.num_mcs = 4, 6, 3
    io.mcs_bits[0], io.mcs_bits[1], io.mcs_bits[2] = 2, 4, 6
    io.dmrs_symbol_mask = (1 << 2) | (1 << 11)
    io.k = 64
    io.no, io.err_var, io.llr_clip = 0.1, 0.0, 20.0
    io.y = io.h = io.active = io.mcs = io.llr = 4096
    for k, v in kw.items():
        if k.startswith("mcs_bits"):
            io.mcs_bits[int(k[8:])] = v
        else:
            setattr(io, k, v)
    return io


def test_exports_and_binding():
    assert "nrx_kbest_detect" in _lib.EXPORTS and "nrx_kbest_workspace_size" in _lib.EXPORTS
    # nrx_kbest_io of include/nrx.h: 17 int32 (7 scalars, mcs_bits[8], mask, k), 4 bytes of
    # alignment, 3 doubles, 5 pointers
    assert ctypes.sizeof(_lib.nrx_kbest_io) == 17 * 4 + 4 + 3 * 8 + 5 * 8
    assert _lib.nrx_kbest_io.k.offset == 64 and _lib.nrx_kbest_io.no.offset == 72
    assert _lib.nrx_kbest_io.llr_clip.offset == 88 and _lib.nrx_kbest_io.y.offset == 96
    # the fields of nrx_lmmse_io, in its order, with k in the place of its padding
    lm = [n for n, _ in _lib.nrx_lmmse_io._fields_ if n != "pad_"]
    kb = [n for n, _ in _lib.nrx_kbest_io._fields_ if n not in ("k", "llr_clip")]
    assert lm == kb


def test_api_version_is_unchanged(lib):
    assert lib.nrx_api_version() == 7


ARG_CASES = [
    (dict(y=None), INVALID_ARG, b"null"), (dict(h=None), INVALID_ARG, b"null"),
    (dict(active=None), INVALID_ARG, b"null"), (dict(llr=None), INVALID_ARG, b"null"),
    (dict(no=0.0), INVALID_ARG, b"no"), (dict(no=-1.0), INVALID_ARG, b"no"),
    (dict(no=float("nan")), INVALID_ARG, b"no"), (dict(err_var=-1e-9), INVALID_ARG, b"err_var"),
    (dict(llr_clip=0.0), INVALID_ARG, b"llr_clip"), (dict(llr_clip=-20.0), INVALID_ARG, b"llr_clip"),
    (dict(llr_clip=float("nan")), INVALID_ARG, b"llr_clip"),
    (dict(k=0), INVALID_ARG, b"k must"), (dict(k=65), INVALID_ARG, b"k must"), (dict(k=-1), INVALID_ARG, b"k must"),
    (dict(mcs_bits1=3), INVALID_ARG, b"mcs_bits"), (dict(mcs_bits0=8), INVALID_ARG, b"mcs_bits"),
    (dict(mcs_bits2=0), INVALID_ARG, b"mcs_bits"),
    (dict(num_symbols=12), SHAPE, b"num_symbols"), (dict(num_tx=0), SHAPE, b"num_tx"),
    (dict(num_rx_ant=0), SHAPE, b"num_rx_ant"), (dict(num_rx_ant=17), SHAPE, b"num_rx_ant"),
    (dict(bits_stride=5), SHAPE, b"bits_stride"), (dict(num_mcs=0), SHAPE, b"num_mcs"),
    (dict(num_mcs=9), SHAPE, b"num_mcs"), (dict(batch=0), SHAPE, b"batch"), (dict(batch=65536), SHAPE, b"batch"),
    (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"), (dict(num_subcarriers=3301), SHAPE, b"num_subcarriers"),
    (dict(num_tx=9), UNSUPPORTED, b"num_tx"), (dict(num_tx=16), UNSUPPORTED, b"num_tx"),
]


@pytest.mark.parametrize("kw,code,word", ARG_CASES)
def test_argument_checks(lib, kw, code, word):
    io = _io(**kw)
    assert lib.nrx_kbest_detect(ctypes.byref(io), 4096, 1 << 40, None) == code
    assert word in lib.nrx_last_error()
    n = ctypes.c_size_t(0)
    assert lib.nrx_kbest_workspace_size(ctypes.byref(io), ctypes.byref(n)) == code


def test_null_io_workspace_and_bytes(lib):
    n = ctypes.c_size_t(0)
    assert lib.nrx_kbest_detect(None, 4096, 1 << 40, None) == INVALID_ARG
    assert lib.nrx_kbest_workspace_size(None, ctypes.byref(n)) == INVALID_ARG
    io = _io()
    assert lib.nrx_kbest_workspace_size(ctypes.byref(io), None) == INVALID_ARG
    assert lib.nrx_kbest_detect(ctypes.byref(io), None, 1 << 40, None) == INVALID_ARG
    assert b"workspace" in lib.nrx_last_error()
    assert lib.nrx_kbest_detect(ctypes.byref(io), 4100, 1 << 40, None) == INVALID_ARG
    assert b"aligned" in lib.nrx_last_error()


def test_workspace_size_and_too_small_workspace(lib):
    sizes = []
    for B in (1, 2, 3, 64, 65535):
        io = _io(batch=B)
        n = ctypes.c_size_t(0)
        assert lib.nrx_kbest_workspace_size(ctypes.byref(io), ctypes.byref(n)) == OK
        sizes.append(n.value)
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    io = _io()
    n = ctypes.c_size_t(0)
    assert lib.nrx_kbest_workspace_size(ctypes.byref(io), ctypes.byref(n)) == OK
    assert lib.nrx_kbest_detect(ctypes.byref(io), 4096, n.value - 1, None) == WORKSPACE
    assert b"workspace too small" in lib.nrx_last_error()
    assert lib.nrx_kbest_detect(ctypes.byref(io), 4096, 0, None) == WORKSPACE


def test_kbest_receiver_rejects_bad_arguments():
    from neural_rx_amd import baseline, chest
    from neural_rx_amd.generator import GenParams
    from neural_rx_amd.kbest import SYSTEMS, KBestBaselineReceiver
    assert SYSTEMS == ("baseline_lmmse_kbest", "baseline_perf_csi_kbest")
    p = GenParams(num_tx=2, num_subcarriers=12, num_rx_ant=4)
    for system in baseline.SYSTEMS + chest.SYSTEMS:
        with pytest.raises(ValueError):
            KBestBaselineReceiver(system, p)
    assert len(baseline.SYSTEMS + chest.SYSTEMS) == 4
    for system in SYSTEMS:
        with pytest.raises(ValueError):
            KBestBaselineReceiver(system, GenParams(num_tx=9, num_subcarriers=12, num_rx_ant=4, cdm_group=(0, 1) * 5))
        for k in (0, 65):
            with pytest.raises(ValueError):
                KBestBaselineReceiver(system, p, k=k)


def test_kbest_receiver_members(lib):
    from neural_rx_amd.evaluate import baseline_note
    from neural_rx_amd.generator import GenParams
    from neural_rx_amd.kbest import KBestBaselineReceiver
    p = GenParams(num_tx=4, num_subcarriers=12, num_rx_ant=4, cdm_group=(0, 1, 0, 1))
    pc = KBestBaselineReceiver("baseline_perf_csi_kbest", p)
    assert pc.perfect_csi and not pc.contaminated and pc.err_var(0.3) == 0.0 and pc.k == 64
    pc.set_covariance(None, None)                                    # accepted and ignored
    assert baseline_note("perf_csi_kbest", pc) is None
    est = KBestBaselineReceiver("baseline_lmmse_kbest", p, k=16)
    assert not est.perfect_csi and est.contaminated and est.k == 16
    assert "pilot-contaminated" in baseline_note("lmmse_kbest", est)
