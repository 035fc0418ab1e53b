"""Host-side checks of the 3-D LMMSE channel estimator: ``chest.lmmse3_design`` (the spectral form)
against the brute-force Kronecker solve of tests/chest3_ref.py and against the 2-D filter, and the
argument checks of ``nrx_chest_lmmse3`` / ``nrx_chest3_workspace_size`` (made before the first HIP
call, so no device is needed)."""
import ctypes

import numpy as np
import pytest

from neural_rx_amd import _lib, chest
from neural_rx_amd.generator import GenParams, ebno_to_no, rx_correlation
from tests import chest3_ref as R3
from tests import chest_ref as R
from tests import synth_chan_ref as C

OK, INVALID_ARG, SHAPE, WORKSPACE = 0, -1, -2, -6
F, A, DMRS = 12, 4, (2, 11)
NO = ebno_to_no(5.0, 2)


def _params(F=F, A=A, dmrs=DMRS, U=2):
    return GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A, dmrs_symbols=dmrs, cdm_group=tuple(u % 2 for u in range(U)))


def _pilots(p, B=2, seed=0):
    """random LS estimates [B, U, F, 14, 2A] float32 and an active mask"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((B, p.num_tx, p.num_subcarriers, 14, 2 * p.num_rx_ant)).astype(np.float32)
    return h, np.ones((B, p.num_tx), np.float32)


@pytest.mark.parametrize("R_s", [rx_correlation(A, 0.9), C.random_psd(A, 5)], ids=["alpha0.9", "complex"])
def test_spectral_estimate_equals_the_kronecker_solve(R_s):
    """F = 12, A = 4, nd = 2, both CDM groups: relative difference below 1e-9"""
    p = _params()
    R_f, R_t = R.model_covariance(F)
    d = chest.lmmse3_design(R_f, R_t, R_s, p, dtype=np.float64)
    h, act = _pilots(p)
    got = R3.lmmse3_apply(h, act, d, DMRS, p.cdm_group, NO)
    ref = R3.lmmse3_brute(h, act, R_f, R_t, R_s, DMRS, p.cdm_group, NO)
    assert np.abs(ref).max() > 0.1
    assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max()


@pytest.mark.parametrize("no", [NO, 10.0 * NO, 0.01 * NO])
def test_error_map_equals_the_kronecker_error(no):
    """err_var(no) = diag(C_hh - W C^H), for several noise levels of one design"""
    p = _params()
    R_f, R_t = R.model_covariance(F)
    R_s = C.random_psd(A, 6)
    d = chest.lmmse3_design(R_f, R_t, R_s, p)
    ev = d.err_var(no)
    assert ev.shape == (2, A, F, 14)
    for g in (0, 1):
        ref = R3.err_brute(R_f, R_t, R_s, DMRS, g, no)
        assert np.abs(ev[g] - ref).max() <= 1e-9 * ref.max()
        assert ev[g].min() > 0 and np.all(ev[g] <= d.prior[:, None, None] * (1 + 1e-12))
    with pytest.raises(ValueError):
        d.err_var(0.0)


@pytest.mark.parametrize("dmrs", [(2, 11), (2,), (2, 7, 11), (2, 3, 10, 11)])
def test_identity_space_covariance_gives_the_2d_filter(dmrs):
    p = _params(F=13, A=2, dmrs=dmrs)
    R_f, R_t = R.model_covariance(13)
    d = chest.lmmse3_design(R_f, R_t, np.eye(2), p, dtype=np.float64)
    h, act = _pilots(p, seed=1)
    got = R3.lmmse3_apply(h, act, d, dmrs, p.cdm_group, NO)
    ref = R.lmmse_brute(h, act, R_f, R_t, dmrs, p.cdm_group, NO)
    assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max()
    # and the error map is the 2-D design's, for every antenna
    ev2 = chest.lmmse_design(R_f, R_t, p, NO).err_var
    assert np.abs(d.err_var(NO) - ev2[:, None]).max() <= 1e-9


def test_design_tables():
    p = _params(F=13, A=3)
    R_f, R_t = R.model_covariance(13)
    R_s = C.random_psd(3, 2)
    d = chest.lmmse3_design(R_f, 3.0 * R_t, 5.0 * R_s, p)          # the scale of R_t and R_s is normalised away
    e = chest.lmmse3_design(R_f, R_t, R_s, p)
    for k in chest.LMMSE3_TABLES:
        a, b = getattr(d, k), getattr(e, k)
        assert a.dtype == np.float32 and a.flags.c_contiguous and np.allclose(a, b, atol=1e-6), k
    assert d.qh.shape == (2, 7, 7, 2) and d.gf.shape == (2, 13, 7, 2) and d.nu.shape == (2, 7)
    assert d.tcoef.shape == (2, 14, 2) and d.vconj.shape == (2, 2, 2) and d.lam.shape == (2,)
    assert d.vs.shape == (3, 3, 2) and d.mu.shape == (3,)
    # group 1 has 6 pilots at F = 13: its tables are zero-padded
    assert not d.qh[1, 6].any() and not d.qh[1, :, 6].any() and not d.gf[1, :, 6].any() and d.nu[1, 6] == 0
    assert np.isclose(d.mu.sum(), 3.0, atol=1e-5) and np.isclose(d.lam.sum(), 2.0, atol=1e-5)
    assert np.abs(d.vs[..., 1]).max() > 0.05                       # a complex V_s
    with pytest.raises(ValueError):
        chest.lmmse3_design(R_f, R_t, np.eye(4), p)
    with pytest.raises(ValueError):
        chest.lmmse3_design(R_f[:12, :12], R_t, R_s, p)


def test_3d_filter_halves_the_error_at_high_correlation():
    """the figure of the issue: at A = 4, alpha = 0.9, 5 dB the exact 3-D filter has about half the
    MSE of the 2-D one that ignores R_s (model covariance, F = 48)"""
    p = _params(F=48)
    R_f, R_t = R.model_covariance(48)
    R_s = rx_correlation(4, 0.9)
    data = [t for t in range(14) if t not in DMRS]
    e3 = chest.lmmse3_design(R_f, R_t, R_s, p).err_var(NO)[:, :, :, data].mean()
    e2 = chest.lmmse_design(R_f, R_t, p, NO).err_var[:, :, data].mean()
    assert 0.4 < e3 / e2 < 0.6, e3 / e2


# ---- the library's argument checks (host only) ----------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


TABLES = ["qh", "gf", "nu", "tcoef", "vconj", "lam", "vs", "mu"]


def _io(**kw):
    """A valid descriptor whose pointers are non-null but never dereferenced on the host"""
    io = _lib.nrx_chest3_io()
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = 2, 2, 24, 14
    io.num_rx_ant, io.num_dmrs_symbols = 4, 2
    io.dmrs_symbols[0], io.dmrs_symbols[1] = 2, 11
    io.cdm_group[0], io.cdm_group[1] = 0, 1
    io.no = 0.1
    io.h_hat = io.active = io.h_out = 4096
    for t in TABLES:
        setattr(io, t, 4096)
    for k, v in kw.items():
        if k.startswith("dmrs_symbols"):
            io.dmrs_symbols[int(k[12:])] = v
        elif k.startswith("cdm_group"):
            io.cdm_group[int(k[9:])] = v
        else:
            setattr(io, k, v)
    return io


SHAPE_CASES = [
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
POINTER_CASES = [(dict(h_hat=None), INVALID_ARG, b"null"), (dict(active=None), INVALID_ARG, b"null"),
                 (dict(h_out=None), INVALID_ARG, b"null"),
                 (dict(no=0.0), INVALID_ARG, b"no"), (dict(no=-1.0), INVALID_ARG, b"no"),
                 (dict(no=float("nan")), INVALID_ARG, b"no"), (dict(no=float("inf")), INVALID_ARG, b"no"),
                 (dict(qh=4100), INVALID_ARG, b"aligned"), (dict(gf=4100), INVALID_ARG, b"aligned")] + \
                [({t: None}, INVALID_ARG, b"null") for t in TABLES]


@pytest.mark.parametrize("kw,code,word", SHAPE_CASES + POINTER_CASES)
def test_chest3_argument_checks(lib, kw, code, word):
    io = _io(**kw)
    assert lib.nrx_chest_lmmse3(ctypes.byref(io), 4096, 1 << 40, None) == code
    assert word in lib.nrx_last_error()


@pytest.mark.parametrize("kw,code,word", SHAPE_CASES)
def test_chest3_workspace_size_checks_the_shape(lib, kw, code, word):
    n = ctypes.c_size_t()
    assert lib.nrx_chest3_workspace_size(ctypes.byref(_io(**kw)), ctypes.byref(n)) == code
    assert word in lib.nrx_last_error()


def test_chest3_workspace(lib):
    io, n = _io(), ctypes.c_size_t()
    assert lib.nrx_chest3_workspace_size(ctypes.byref(io), ctypes.byref(n)) == OK
    assert n.value == 2 * 2 * 12 * 2 * 8 * 4         # B U Pmax nd 2A floats
    bare = _io(h_hat=None, active=None, h_out=None, no=0.0, **{t: None for t in TABLES})
    m = ctypes.c_size_t()
    assert lib.nrx_chest3_workspace_size(ctypes.byref(bare), ctypes.byref(m)) == OK and m.value == n.value
    big = ctypes.c_size_t()
    assert lib.nrx_chest3_workspace_size(ctypes.byref(_io(batch=3)), ctypes.byref(big)) == OK and big.value > n.value
    assert lib.nrx_chest3_workspace_size(ctypes.byref(io), None) == INVALID_ARG
    assert lib.nrx_chest3_workspace_size(None, ctypes.byref(n)) == INVALID_ARG
    assert lib.nrx_chest_lmmse3(None, 4096, n, None) == INVALID_ARG
    assert lib.nrx_chest_lmmse3(ctypes.byref(io), None, n, None) == INVALID_ARG
    assert lib.nrx_chest_lmmse3(ctypes.byref(io), 4098, n, None) == INVALID_ARG and b"aligned" in lib.nrx_last_error()
    assert lib.nrx_chest_lmmse3(ctypes.byref(io), 4096, n.value - 1, None) == WORKSPACE
    assert b"workspace" in lib.nrx_last_error()


def test_binding_and_python_checks():
    for s in ("nrx_chest3_workspace_size", "nrx_chest_lmmse3"):
        assert s in _lib.EXPORTS
    # 26 int32 (6 scalars, dmrs_symbols[4], cdm_group[16]), 1 double, 11 pointers
    assert ctypes.sizeof(_lib.nrx_chest3_io) == 26 * 4 + 8 + 11 * 8
    assert _lib.nrx_chest3_io.no.offset == 104 and _lib.nrx_chest3_io.h_hat.offset == 112
    assert _lib.nrx_chest3_io.qh.offset == 128 and _lib.nrx_chest3_io.h_out.offset == 192
    assert "lmmse3" in chest.KINDS
