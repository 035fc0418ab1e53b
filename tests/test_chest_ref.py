"""The host side of the channel-estimation baselines: the filter design of
``neural_rx_amd/chest.py`` against the brute-force statement of tests/chest_ref.py, the linear
interpolator's definition, and the argument checks of ``nrx_cov_accumulate`` / ``nrx_chest_lmmse`` /
``nrx_chest_lin`` (they run before the first HIP call, so their status codes are checked here
through the real ``libnrx.so``); no GPU.
"""
import ctypes

import numpy as np
import pytest

from neural_rx_amd import _lib
from neural_rx_amd.generator import GenParams

from tests import chest_ref as R

OK, INVALID_ARG, SHAPE, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3, -6
NO = 0.23


def _cx(a):
    return a[..., 0] + 1j * a[..., 1]


@pytest.mark.parametrize("F", [13, 24])
@pytest.mark.parametrize("dmrs", [(2,), (2, 11), (2, 7, 11), (2, 3, 10, 11)])
def test_eigen_design_equals_the_kronecker_solve(F, dmrs):
    """chest.lmmse_design (nd frequency filters on the eigenvectors of R_t[D, D]) is the brute-force
    2-D filter, and its error map the brute-force one, to 1e-10"""
    from neural_rx_amd.chest import lmmse_design
    R_f, R_t = R.model_covariance(F)
    R_f, R_t = 1.1 * R_f, 0.9 * R_t                     # neither diagonal is 1
    p = GenParams(num_tx=2, num_subcarriers=F, num_rx_ant=2, dmrs_symbols=dmrs)
    d = lmmse_design(R_f, R_t, p, NO, dtype=np.float64)
    W, a, v = _cx(d.filt), _cx(d.tcoef), _cx(d.vconj)
    for g in (0, 1):
        P = R.pilots(F, g)
        full = np.einsum("kt,kd,kfp->ftdp", a, v, W[g][:, :, :len(P)])
        brute, err = R.lmmse_filter_brute(R_f, R_t, dmrs, g, NO)
        assert np.abs(full - brute).max() <= 1e-10
        assert np.abs(d.err_var[g] - err).max() <= 1e-10
        assert np.all(W[g][:, :, len(P):] == 0)        # group 1 of an odd F is zero-padded
        assert err.min() > 0 and err.max() < R_f[0, 0].real
    r32 = lmmse_design(R_f, R_t, p, NO)
    assert r32.filt.dtype == np.float32 and r32.filt.shape == (2, len(dmrs), F, (F + 1) // 2, 2)
    assert np.array_equal(r32.filt, d.filt.astype(np.float32))
    assert r32.tcoef.shape == (len(dmrs), 14, 2) and r32.vconj.shape == (len(dmrs), len(dmrs), 2)


def test_tables_applied_equal_the_brute_force_estimate():
    """chest_ref.lmmse_apply on unrounded tables = the Kronecker filter applied to the pilots"""
    from neural_rx_amd.chest import lmmse_design
    F, dmrs, groups = 13, (2, 11), (0, 1, 1)
    rng = np.random.default_rng(0)
    h_hat = rng.standard_normal((2, 3, F, 14, 4)).astype(np.float32)
    active = np.array([[1, 1, 0], [1, 0, 1]], np.float32)
    R_f, R_t = R.model_covariance(F)
    p = GenParams(num_tx=3, num_subcarriers=F, num_rx_ant=2, dmrs_symbols=dmrs, cdm_group=groups)
    d = lmmse_design(R_f, R_t, p, NO, dtype=np.float64)
    got = R.lmmse_apply(h_hat, active, d.filt, d.tcoef, d.vconj, dmrs, groups)
    ref = R.lmmse_brute(h_hat, active, R_f, R_t, dmrs, groups, NO)
    assert np.abs(got - ref).max() <= 1e-10
    assert np.all(got[0, 2] == 0) and np.all(got[1, 1] == 0)


@pytest.mark.parametrize("F,dmrs,groups", [(13, (2, 11), (0, 1)), (12, (3, 6, 9, 12), (1, 0)), (24, (0, 13), (0, 1))])
def test_linear_interpolator_reproduces_an_affine_channel(F, dmrs, groups):
    """h = a + b f + c t at the pilots -> the same plane everywhere, extrapolated edges included"""
    rng = np.random.default_rng(1)
    A = 2
    a, b, c = (rng.standard_normal((A,)) + 1j * rng.standard_normal((A,)) for _ in range(3))
    f, t = np.arange(F)[:, None, None], np.arange(14)[None, :, None]
    plane = a + b * f + c * t                                                  # [F, T, A]
    truth = np.broadcast_to(R.to_channels(plane), (1, 2, F, 14, 2 * A))
    h_hat = np.full((1, 2, F, 14, 2 * A), np.nan)
    for u, g in enumerate(groups):                                             # only the own pilots are read
        for tt in dmrs:
            h_hat[0, u, g::2, tt] = truth[0, u, g::2, tt]
    out = R.lin_interp(h_hat, np.ones((1, 2)), dmrs, groups)
    assert np.abs(out - truth).max() <= 1e-12


def test_linear_interpolator_repeats_a_single_pilot_or_symbol():
    rng = np.random.default_rng(2)
    h_hat = rng.standard_normal((1, 1, 2, 14, 2))
    out = R.lin_interp(h_hat, np.ones((1, 1)), (5,), (1,))                     # F = 2, group 1: one pilot
    assert np.all(out == h_hat[:, :, 1:2, 5:6])
    assert np.all(R.lin_interp(h_hat, np.zeros((1, 1)), (5,), (1,)) == 0)


def test_lags_and_toeplitz():
    from neural_rx_amd.chest import toeplitz
    rng = np.random.default_rng(3)
    h = rng.standard_normal((2, 2, 5, 14, 4)).astype(np.float32)
    sf, st = R.lag_sums(h)
    hc = R.to_complex(h)
    assert np.isclose(sf[0], np.sum(np.abs(hc) ** 2)) and np.isclose(st[0], sf[0])
    assert np.isclose(sf[4], np.sum(hc[:, :, 4] * np.conj(hc[:, :, 0])))
    assert np.isclose(st[13], np.sum(hc[:, :, :, 13] * np.conj(hc[:, :, :, 0])))
    Rm = toeplitz(sf)
    assert np.array_equal(Rm, R.toeplitz(sf)) and np.array_equal(Rm, Rm.conj().T) and Rm[3, 1] == sf[2]
    nf, nt = R.lag_counts(2, 2, 5, 2)
    assert nf[0] == nt[0] == hc.size and nf[4] == 2 * 2 * 2 * 14 and nt[13] == 2 * 2 * 2 * 5


# ---- the library's argument checks (host only) ----------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def _chest(**kw):
    """A valid descriptor whose pointers are non-null but never dereferenced on the host: every
    case below must be rejected before the first HIP call."""
    io = _lib.nrx_chest_io()
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = 2, 2, 24, 14
    io.num_rx_ant, io.num_dmrs_symbols = 4, 2
    io.dmrs_symbols[0], io.dmrs_symbols[1] = 2, 11
    io.cdm_group[0], io.cdm_group[1] = 0, 1
    io.no = 0.1
    io.h_hat = io.active = io.filt = io.tcoef = io.vconj = io.h_out = 4096
    for k, v in kw.items():
        if k.startswith("dmrs_symbols"):
            io.dmrs_symbols[int(k[12:])] = v
        elif k.startswith("cdm_group"):
            io.cdm_group[int(k[9:])] = v
        else:
            setattr(io, k, v)
    return io


COMMON = [
    (dict(h_hat=None), INVALID_ARG, b"null"), (dict(active=None), INVALID_ARG, b"null"),
    (dict(h_out=None), INVALID_ARG, b"null"),
    (dict(no=0.0), INVALID_ARG, b"no"), (dict(no=-1.0), INVALID_ARG, b"no"), (dict(no=float("nan")), INVALID_ARG, b"no"),
    (dict(num_symbols=12), SHAPE, b"num_symbols"),
    (dict(num_dmrs_symbols=0), SHAPE, b"num_dmrs_symbols"), (dict(num_dmrs_symbols=5), SHAPE, b"num_dmrs_symbols"),
    (dict(dmrs_symbols1=14), INVALID_ARG, b"dmrs_symbols"), (dict(dmrs_symbols0=-1), INVALID_ARG, b"dmrs_symbols"),
    (dict(dmrs_symbols1=2), INVALID_ARG, b"dmrs_symbols"),
    (dict(cdm_group0=2), INVALID_ARG, b"cdm_group"), (dict(cdm_group1=-1), INVALID_ARG, b"cdm_group"),
    (dict(num_rx_ant=0), SHAPE, b"num_rx_ant"), (dict(num_rx_ant=17), SHAPE, b"num_rx_ant"),
    (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"), (dict(num_subcarriers=3301), SHAPE, b"num_subcarriers"),
    (dict(batch=0), SHAPE, b"batch"), (dict(num_tx=0), SHAPE, b"num_tx"), (dict(num_tx=17), SHAPE, b"num_tx"),
    (dict(batch=65536), SHAPE, b"batch"),
]
LMMSE_ONLY = [(dict(filt=None), INVALID_ARG, b"null"), (dict(tcoef=None), INVALID_ARG, b"null"),
              (dict(vconj=None), INVALID_ARG, b"null"), (dict(filt=4100), INVALID_ARG, b"aligned")]


@pytest.mark.parametrize("kw,code,word", COMMON + LMMSE_ONLY)
def test_chest_lmmse_argument_checks(lib, kw, code, word):
    io = _chest(**kw)
    assert lib.nrx_chest_lmmse(ctypes.byref(io), None) == code
    assert word in lib.nrx_last_error()


@pytest.mark.parametrize("kw,code,word", COMMON)
def test_chest_lin_argument_checks(lib, kw, code, word):
    io = _chest(filt=None, tcoef=None, vconj=None, **kw)       # the tables are not read
    assert lib.nrx_chest_lin(ctypes.byref(io), None) == code
    assert word in lib.nrx_last_error()


def _cov(**kw):
    io = _lib.nrx_cov_io()
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols, io.num_rx_ant = 2, 2, 24, 14, 4
    io.h = io.acc = 4096
    for k, v in kw.items():
        setattr(io, k, v)
    return io


@pytest.mark.parametrize("kw,code,word", [
    (dict(h=None), INVALID_ARG, b"null"), (dict(acc=None), INVALID_ARG, b"null"),
    (dict(num_symbols=13), SHAPE, b"num_symbols"), (dict(batch=0), SHAPE, b"batch"),
    (dict(num_tx=0), SHAPE, b"num_tx"), (dict(num_tx=17), SHAPE, b"num_tx"),
    (dict(num_rx_ant=0), SHAPE, b"num_rx_ant"), (dict(num_rx_ant=17), SHAPE, b"num_rx_ant"),
    (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"), (dict(num_subcarriers=3301), SHAPE, b"num_subcarriers"),
])
def test_cov_argument_checks(lib, kw, code, word):
    io = _cov(**kw)
    n = ctypes.c_size_t(1 << 30)
    assert lib.nrx_cov_accumulate(ctypes.byref(io), 4096, n, None) == code
    assert word in lib.nrx_last_error()
    assert lib.nrx_cov_workspace_size(ctypes.byref(io), ctypes.byref(n)) == code


def test_cov_workspace(lib):
    io, n = _cov(), ctypes.c_size_t()
    assert lib.nrx_cov_workspace_size(ctypes.byref(io), ctypes.byref(n)) == OK
    assert n.value > 0 and n.value % ((24 + 14) * 16) == 0
    assert lib.nrx_cov_workspace_size(ctypes.byref(io), None) == INVALID_ARG
    assert lib.nrx_cov_accumulate(ctypes.byref(io), None, n, None) == INVALID_ARG
    assert lib.nrx_cov_accumulate(ctypes.byref(io), 4096, n.value - 1, None) == WORKSPACE
    assert b"workspace" in lib.nrx_last_error()


def test_null_io(lib):
    assert lib.nrx_chest_lmmse(None, None) == INVALID_ARG
    assert lib.nrx_chest_lin(None, None) == INVALID_ARG
    assert lib.nrx_cov_accumulate(None, 4096, 1 << 20, None) == INVALID_ARG
    assert lib.nrx_last_error()


def test_exports_and_binding():
    for s in ("nrx_cov_workspace_size", "nrx_cov_accumulate", "nrx_chest_lmmse", "nrx_chest_lin"):
        assert s in _lib.EXPORTS
    # nrx_cov_io: 6 int32, 2 pointers; nrx_chest_io: 26 int32 (6 scalars, dmrs_symbols[4],
    # cdm_group[16]), 1 double, 6 pointers
    assert ctypes.sizeof(_lib.nrx_cov_io) == 6 * 4 + 2 * 8 and _lib.nrx_cov_io.h.offset == 24
    assert ctypes.sizeof(_lib.nrx_chest_io) == 26 * 4 + 8 + 6 * 8
    assert _lib.nrx_chest_io.no.offset == 104 and _lib.nrx_chest_io.h_hat.offset == 112


def test_receiver_rejects_bad_arguments():
    from neural_rx_amd import baseline, chest
    assert baseline.SYSTEMS == ("baseline_lsnn_lmmse", "baseline_perf_csi_lmmse")
    assert chest.SYSTEMS == ("baseline_lslin_lmmse", "baseline_lmmse_lmmse")
    p = GenParams(num_tx=2, num_subcarriers=12, num_rx_ant=4)
    for bad in ("baseline_lsnn_lmmse", "baseline_lmmse_kbest", "lmmse_lmmse"):
        with pytest.raises(ValueError):
            chest.EstimatorBaselineReceiver(bad, p)
    with pytest.raises(ValueError):
        chest.EstimatorBaselineReceiver("baseline_lslin_lmmse", GenParams(num_tx=9, num_subcarriers=12, num_rx_ant=4,
                                                                          cdm_group=(0, 1) * 5))
    with pytest.raises(ValueError):
        chest.ChannelEstimator("nn", p)
    with pytest.raises(ValueError):
        chest.lmmse_design(np.eye(12), np.eye(14), p, 0.0)
    with pytest.raises(ValueError):
        chest.lmmse_design(np.eye(11), np.eye(14), p, 0.1)


@pytest.mark.parametrize("groups,active,expect", [((0, 1), None, False), ((0, 1, 0, 1), 1, False),
                                                  ((0, 1, 0, 1), 2, True), ((0, 0), None, True)])
def test_contamination_and_err_var(lib, groups, active, expect):
    from neural_rx_amd import chest
    p = GenParams(num_tx=len(groups), num_subcarriers=12, num_rx_ant=4, cdm_group=groups, num_active=active)
    lin = chest.EstimatorBaselineReceiver("baseline_lslin_lmmse", p)
    assert lin.contaminated is expect and not lin.perfect_csi
    na = len(groups) if active is None else active
    assert lin.err_var(0.2) == na * 0.1
    R_f, R_t = R.model_covariance(12)
    rx = chest.EstimatorBaselineReceiver("baseline_lmmse_lmmse", p, R_f=R_f, R_t=R_t)
    d = chest.lmmse_design(R_f, R_t, p, 0.2)
    data = [t for t in range(14) if t not in (2, 11)]
    want = na * np.mean([d.err_var[g][:, data].mean() for g in groups])
    assert rx.err_var(0.2) == pytest.approx(want, rel=1e-12) and 0 < want < na * 0.1
    with pytest.raises(ValueError):
        chest.EstimatorBaselineReceiver("baseline_lmmse_lmmse", p).err_var(0.2)    # no covariance
