"""The numpy LMMSE + max-log reference (tests/lmmse_ref.py) and the host side of
``nrx_lmmse_detect``; no GPU.

The reference is pinned three ways: its bit-error counts on the oracle generator's slots (the
table of tests/lmmse_ref.CASES: a wrong sign convention, bit-to-axis mapping or active masking
moves them), a closed form for one user and one antenna, and exact zeros where the contract says
zero.  The argument checks of the library run before its first HIP call, so their status codes
are checked here through the real ``libnrx.so``.
"""
import ctypes
import functools

import numpy as np
import pytest

from neural_rx_amd import _lib
from oracle import synth_ref as S

from tests import lmmse_ref as R

OK, INVALID_ARG, SHAPE, UNSUPPORTED = 0, -1, -2, -3


@functools.lru_cache(maxsize=None)
def _slots(name):
    return S.generate(R.case_spec(name))


@pytest.mark.parametrize("name,csi", [(n, c) for n in R.CASES for c in R.CASES[n][9]])
def test_reference_counts(name, csi):
    spec, g = R.case_spec(name), _slots(name)
    llr = R.lmmse_detect(g.y, g.h_hat if csi == "ls" else g.h, g.active, g.mcs, spec.mcs_bits, spec.no,
                         spec.dmrs_symbols)
    cnt = S.count_errors(llr, g.bits, g.mcs, spec.mcs_bits, g.active, spec.dmrs_symbols).sum(0)
    assert (int(cnt[0]), int(cnt[1])) == R.CASES[name][9][csi]


@pytest.mark.parametrize("m", [2, 4, 6])
def test_single_user_single_antenna_is_maxlog_on_y_over_h(m):
    """U = 1, A = 1: the unbiased estimate is y / h and the noise no / |h|^2, so the LLRs are the
    direct max-log over the constellation."""
    rng = np.random.default_rng(m)
    B, F, T, no = 2, 5, 14, 0.07
    h = rng.standard_normal((B, 1, F, T, 2)).astype(np.float32)
    y = rng.standard_normal((B, F, T, 2)).astype(np.float32)
    llr = R.lmmse_detect(y, h, np.ones((B, 1), np.float32), None, (m,), no, ())
    hc = h[:, 0, ..., 0].astype(np.float64) + 1j * h[:, 0, ..., 1]
    yc = y[..., 0].astype(np.float64) + 1j * y[..., 1]
    d = np.abs((yc / hc)[..., None] - R.constellation(m)) ** 2 * (np.abs(hc) ** 2 / no)[..., None]
    lab = np.arange(1 << m)
    for k in range(m):
        one = ((lab >> k) & 1).astype(bool)
        np.testing.assert_allclose(llr[0, :, 0, ..., k], d[..., ~one].min(-1) - d[..., one].min(-1),
                                   rtol=1e-9, atol=1e-9)


def test_constellation_matches_the_generator():
    for m in (2, 4, 6):
        pts = R.constellation(m)
        assert abs(np.mean(np.abs(pts) ** 2) - 1.0) < 1e-12
        # even label bits move the real axis only, odd ones the imaginary axis only
        for k in range(m):
            moved = pts[np.arange(1 << m) ^ (1 << k)] - pts
            assert np.all((moved.imag if k % 2 == 0 else moved.real) == 0)


def test_zeros_for_inactive_dmrs_and_unused_bits():
    spec, g = R.case_spec("C3"), _slots("C3")
    llr = R.lmmse_detect(g.y, g.h, g.active, g.mcs, spec.mcs_bits, spec.no, spec.dmrs_symbols)[0]
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
    llr = R.lmmse_detect(y, np.zeros((1, 2, 3, 14, 8), np.float32), np.ones((1, 2), np.float32), None, (4,), 0.1, (2,))
    assert np.all(llr == 0)


# ---- the library's argument checks (host only) ----------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def _io(**kw):
    """A valid descriptor whose pointers are non-null but never dereferenced on the host: every
    case below must be rejected before the first HIP call."""
    io = _lib.nrx_lmmse_io()
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = 2, 2, 12, 14
    io.num_rx_ant, io.bits_stride, io.num_mcs = 4, 6, 3
    io.mcs_bits[0], io.mcs_bits[1], io.mcs_bits[2] = 2, 4, 6
    io.dmrs_symbol_mask = (1 << 2) | (1 << 11)
    io.no, io.err_var = 0.1, 0.0
    io.y = io.h = io.active = io.mcs = io.llr = 4096
    for k, v in kw.items():
        if k.startswith("mcs_bits"):
            io.mcs_bits[int(k[8:])] = v
        else:
            setattr(io, k, v)
    return io


def test_exports_and_binding():
    assert "nrx_lmmse_detect" in _lib.EXPORTS
    # nrx_lmmse_io of include/nrx.h: 17 int32 (7 scalars, mcs_bits[8], mask, pad_), 4 bytes of
    # alignment, 2 doubles, 5 pointers
    assert ctypes.sizeof(_lib.nrx_lmmse_io) == 17 * 4 + 4 + 2 * 8 + 5 * 8
    assert _lib.nrx_lmmse_io.no.offset == 72 and _lib.nrx_lmmse_io.y.offset == 88


@pytest.mark.parametrize("kw,code,word", [
    (dict(y=None), INVALID_ARG, b"null"), (dict(h=None), INVALID_ARG, b"null"),
    (dict(active=None), INVALID_ARG, b"null"), (dict(llr=None), INVALID_ARG, b"null"),
    (dict(no=0.0), INVALID_ARG, b"no"), (dict(no=-1.0), INVALID_ARG, b"no"),
    (dict(no=float("nan")), INVALID_ARG, b"no"), (dict(err_var=-1e-9), INVALID_ARG, b"err_var"),
    (dict(mcs_bits1=3), INVALID_ARG, b"mcs_bits"), (dict(mcs_bits0=8), INVALID_ARG, b"mcs_bits"),
    (dict(mcs_bits2=0), INVALID_ARG, b"mcs_bits"),
    (dict(num_symbols=12), SHAPE, b"num_symbols"), (dict(num_tx=0), SHAPE, b"num_tx"),
    (dict(num_rx_ant=0), SHAPE, b"num_rx_ant"), (dict(num_rx_ant=17), SHAPE, b"num_rx_ant"),
    (dict(bits_stride=5), SHAPE, b"bits_stride"), (dict(num_mcs=0), SHAPE, b"num_mcs"),
    (dict(num_mcs=9), SHAPE, b"num_mcs"), (dict(batch=0), SHAPE, b"batch"),
    (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"),
    (dict(num_tx=9), UNSUPPORTED, b"num_tx"), (dict(num_tx=16), UNSUPPORTED, b"num_tx"),
])
def test_argument_checks(lib, kw, code, word):
    io = _io(**kw)
    assert lib.nrx_lmmse_detect(ctypes.byref(io), None) == code
    assert word in lib.nrx_last_error()


def test_null_io(lib):
    assert lib.nrx_lmmse_detect(None, None) == INVALID_ARG
    assert lib.nrx_last_error()


def test_baseline_receiver_rejects_bad_arguments():
    from neural_rx_amd.baseline import SYSTEMS, BaselineReceiver
    from neural_rx_amd.generator import GenParams
    assert SYSTEMS == ("baseline_lsnn_lmmse", "baseline_perf_csi_lmmse")
    with pytest.raises(ValueError):
        BaselineReceiver("baseline_lmmse_kbest", GenParams(num_tx=2, num_subcarriers=12, num_rx_ant=4))
    with pytest.raises(ValueError):
        BaselineReceiver("baseline_perf_csi_lmmse", GenParams(num_tx=9, num_subcarriers=12, num_rx_ant=4,
                                                              cdm_group=(0, 1) * 5))


@pytest.mark.parametrize("system,users,groups,active,expect", [
    ("baseline_lsnn_lmmse", 2, (0, 1), None, False),          # one port per CDM group
    ("baseline_lsnn_lmmse", 4, (0, 1, 0, 1), 1, False),       # one active port: nothing to collide with
    ("baseline_lsnn_lmmse", 4, (0, 1, 0, 1), 2, True),        # ports 0 and 2 can both be drawn
    ("baseline_lsnn_lmmse", 8, (0, 1) * 4, None, True),
    ("baseline_lsnn_lmmse", 2, (0, 0), None, True),
    ("baseline_perf_csi_lmmse", 8, (0, 1) * 4, None, False),  # the true channel is never contaminated
])
def test_contamination_note(lib, system, users, groups, active, expect):
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.evaluate import baseline_note
    from neural_rx_amd.generator import GenParams
    rx = BaselineReceiver(system, GenParams(num_tx=users, num_subcarriers=12, num_rx_ant=4, cdm_group=groups,
                                            num_active=active))
    assert rx.contaminated is expect
    note = baseline_note("lsnn_lmmse", rx)
    if expect:
        assert note.startswith("lsnn_lmmse: note:") and "pilot-contaminated" in note and "\n" not in note
    else:
        assert note is None
