"""Host-side checks of the correlated per-user channel: the numpy statement tests/synth_chan_ref.py
against oracle/synth_ref.py, ``generator.rx_correlation`` / ``scenario`` / ``GenParams.rx_mix``, and
the argument checks of ``nrx_generate_slots_ex`` and ``nrx_cov_space_accumulate`` (made before the
first HIP call, so no device is needed)."""
import ctypes
import dataclasses

import numpy as np
import pytest

from neural_rx_amd import _lib, generator
from neural_rx_amd.generator import GenParams
from oracle import synth_ref as S
from tests import synth_chan_ref as C

OK, INVALID_ARG, SHAPE, WORKSPACE = 0, -1, -2, -6


def _spec(**kw):
    base = dict(batch=2, num_tx=3, num_subcarriers=12, num_rx_ant=2, cdm_group=(0, 1, 0), mcs_bits=(2, 4),
                mcs_of_user=(-1, 0, 1), num_active=2, seed=99, slot_offset=5)
    base.update(kw)
    return S.GenSpec(**base)


def test_uniform_profiles_without_mix_equal_the_oracle_exactly():
    s = _spec()
    ref = S.generate(s)
    got = C.generate(s, user_profiles=[(s.max_delay_s, s.max_doppler_hz)] * 3)
    none = C.generate(s)
    for f in dataclasses.fields(S.GenOut):
        a, b, c = getattr(ref, f.name), getattr(got, f.name), getattr(none, f.name)
        assert a.tobytes() == b.tobytes() == c.tobytes(), f.name


def test_profiles_act_on_their_own_port_only():
    s = _spec(num_active=None)
    ref = S.generate(s)
    got = C.generate(s, user_profiles=[(s.max_delay_s, s.max_doppler_hz), (0.0, 0.0), (s.max_delay_s, 50.0)])
    A = s.num_rx_ant
    assert np.array_equal(got.h[:, 0], ref.h[:, 0]) and not np.array_equal(got.h[:, 2], ref.h[:, 2])
    assert np.array_equal(got.bits, ref.bits) and np.array_equal(got.active, ref.active)
    flat = got.h[:, 1, :, :, :A] + 1j * got.h[:, 1, :, :, A:]              # no delay, no Doppler: one value per antenna
    assert np.abs(flat - flat[:, :1, :1]).max() < 1e-6


def test_mixing_is_a_left_multiplication_of_the_taps():
    s = _spec(num_active=None, no=0.0)
    A = s.num_rx_ant
    M = C.hermitian_sqrt(C.random_psd(A, 3))
    assert np.abs(M.imag).max() > 0.05 and not np.allclose(M, M.T)         # complex: M, M^T and conj(M) differ
    ref, got = S.generate(s), C.generate(s, rx_mix=M)
    cx = lambda h: h[..., :A].astype(np.float64) + 1j * h[..., A:]         # noqa: E731
    assert np.abs(cx(got.h) - np.einsum("ac,buftc->bufta", M, cx(ref.h))).max() < 1e-6
    # y and h stay consistent: without noise y = sum_u h_u x_u
    y = np.einsum("bufta,buft->bfta", cx(got.h), got.x)
    assert np.abs(cx(got.y) - y).max() < 2e-6
    eye = C.generate(s, rx_mix=np.eye(A))
    assert np.abs(eye.h - ref.h).max() < 1e-7 and np.array_equal(eye.bits, ref.bits)


# utils/channel_models.py:20-33 of the reference: exponents of alpha along the first row
REF_EXPONENTS = {
    2: [0, 1],
    4: [0, 1 / 9, 4 / 9, 1],
    8: [0, 1 / 49, 4 / 49, 9 / 49, 16 / 49, 25 / 49, 36 / 49, 1],
}


@pytest.mark.parametrize("A", [2, 4, 8])
@pytest.mark.parametrize("alpha", [0.0, 0.3, 0.9])
def test_rx_correlation_equals_the_reference_tables(A, alpha):
    R = generator.rx_correlation(A, alpha)
    row = np.array([1.0 if e == 0 else alpha ** e for e in REF_EXPONENTS[A]])
    ref = np.array([[row[abs(i - j)] for j in range(A)] for i in range(A)])
    assert R.shape == (A, A) and np.allclose(R, ref, rtol=1e-14, atol=0)
    assert np.linalg.eigvalsh(R).min() > -1e-12
    if alpha == 0.0:
        assert np.array_equal(R, np.eye(A))


def test_rx_correlation_other_sizes():
    assert np.array_equal(generator.rx_correlation(1, 0.9), [[1.0]])
    for A in (3, 5, 16):
        R = generator.rx_correlation(A, 0.9)
        assert np.allclose(np.diag(R), 1.0) and np.isclose(R[0, A - 1], 0.9) and np.linalg.eigvalsh(R).min() > -1e-12
    with pytest.raises(ValueError):
        generator.rx_correlation(0, 0.5)
    with pytest.raises(ValueError):
        generator.rx_correlation(4, 1.5)


def test_rms_delay_spread_constant():
    """rms delay spread of p(x) ~ exp(-3 x) on [0, 1] by quadrature: 0.23658"""
    x = (np.arange(200000) + 0.5) / 200000
    w = np.exp(-3.0 * x)
    w /= w.sum()
    m1, m2 = np.sum(w * x), np.sum(w * x * x)
    assert abs(np.sqrt(m2 - m1 * m1) - generator.RMS_OVER_MAX_DELAY) < 1e-5


def test_scenario():
    p = GenParams(num_tx=2, num_subcarriers=24, num_rx_ant=4)
    lo, hi = generator.scenario("double_tdl_low", p), generator.scenario("double_tdl_high", p)
    assert not p.correlated and lo.correlated and hi.correlated
    assert np.array_equal(lo.rx_corr, np.eye(4)) and np.array_equal(hi.rx_corr, generator.rx_correlation(4, 0.9))
    for q in (lo, hi):
        (d0, f0), (d1, f1) = q.profiles()
        assert np.isclose(d0 * 0.23658, 100e-9) and f0 == 400.0 and np.isclose(d1 * 0.23658, 300e-9) and f1 == 100.0
        assert q.num_subcarriers == 24 and q.seed == p.seed
    for n in (1, 3):
        with pytest.raises(ValueError):
            generator.scenario("double_tdl_low", GenParams(num_tx=n, num_subcarriers=24, num_rx_ant=4,
                                                           cdm_group=(0, 1, 0)))
    with pytest.raises(ValueError):
        generator.scenario("double_tdl_medium", p)


def test_rx_mix_is_the_hermitian_square_root():
    R = C.random_psd(3, 11)
    p = GenParams(num_tx=2, num_subcarriers=24, num_rx_ant=3, rx_corr=R)
    M = p.rx_mix()
    assert np.allclose(M, M.conj().T) and np.allclose(M @ M.conj().T, R) and np.allclose(M, C.hermitian_sqrt(R))
    assert GenParams(num_tx=2, num_subcarriers=24, num_rx_ant=3).rx_mix() is None
    assert p.profiles() == [(300e-9, 400.0)] * 2
    for bad in (np.eye(4), np.array([[1, 2, 0], [0, 1, 0], [0, 0, 1.0]]), -np.eye(3)):
        with pytest.raises(ValueError):
            dataclasses.replace(p, rx_corr=bad).rx_mix()
    with pytest.raises(ValueError):
        dataclasses.replace(p, user_profiles=[(1e-7, 10.0)]).profiles()


# ---- the library's argument checks (host only) ----------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def _gen(U=2):
    d = GenParams(num_tx=U, num_subcarriers=24, num_rx_ant=4, cdm_group=tuple(u % 2 for u in range(U))).desc(2, 0.1)
    o = _lib.nrx_gen_out()
    o.y = 4096
    c = _lib.nrx_gen_chan()
    for u in range(16):
        c.max_delay_s[u], c.max_doppler_hz[u] = 1e-7, 100.0
    return d, c, o


def test_binding():
    for s in ("nrx_generate_slots_ex", "nrx_cov_space_workspace_size", "nrx_cov_space_accumulate"):
        assert s in _lib.EXPORTS
    # nrx_gen_chan: 2 x 16 doubles and a pointer -- 264 bytes, passed to the kernels by value
    assert ctypes.sizeof(_lib.nrx_gen_chan) == 264 and _lib.nrx_gen_chan.rx_mix.offset == 256
    assert _lib.nrx_gen_chan.max_doppler_hz.offset == 128
    assert ctypes.sizeof(_lib.nrx_cov_space_io) == 6 * 4 + 2 * 8 and _lib.nrx_cov_space_io.h.offset == 24


@pytest.mark.parametrize("field", ["max_delay_s", "max_doppler_hz"])
@pytest.mark.parametrize("value", [-1e-9, float("nan"), float("inf")])
def test_generate_ex_rejects_bad_spreads(lib, field, value):
    d, c, o = _gen()
    getattr(c, field)[1] = value
    assert lib.nrx_generate_slots_ex(ctypes.byref(d), ctypes.byref(c), ctypes.byref(o), 4096, 1 << 40, None) == INVALID_ARG
    assert b"spread" in lib.nrx_last_error()
    # a port beyond num_tx is not read: the next check (the workspace size) is reached
    d, c, o = _gen()
    getattr(c, field)[2] = value
    assert lib.nrx_generate_slots_ex(ctypes.byref(d), ctypes.byref(c), ctypes.byref(o), 4096, 16, None) == WORKSPACE


def test_generate_ex_keeps_the_checks_of_generate_slots(lib):
    d, c, o = _gen()
    call = lambda: lib.nrx_generate_slots_ex(ctypes.byref(d), ctypes.byref(c), ctypes.byref(o), 4096, 16, None)  # noqa: E731
    assert call() == WORKSPACE                     # everything valid but the workspace size
    assert lib.nrx_generate_slots_ex(ctypes.byref(d), None, ctypes.byref(o), 4096, 16, None) == WORKSPACE
    assert lib.nrx_generate_slots_ex(None, ctypes.byref(c), ctypes.byref(o), 4096, 16, None) == INVALID_ARG
    assert lib.nrx_generate_slots_ex(ctypes.byref(d), ctypes.byref(c), None, 4096, 16, None) == INVALID_ARG
    assert lib.nrx_generate_slots_ex(ctypes.byref(d), ctypes.byref(c), ctypes.byref(o), None, 16, None) == INVALID_ARG
    c.rx_mix = 4100
    assert call() == INVALID_ARG and b"aligned" in lib.nrx_last_error()
    c.rx_mix = 4096
    assert call() == WORKSPACE
    d.num_rx_ant = 17
    assert call() == SHAPE
    d.num_rx_ant, d.num_taps = 4, 9
    assert call() == INVALID_ARG
    # the workspace does not grow with chan
    n = ctypes.c_size_t()
    d.num_taps = 6
    assert lib.nrx_gen_workspace_size(ctypes.byref(d), ctypes.byref(n)) == OK
    assert lib.nrx_generate_slots_ex(ctypes.byref(d), ctypes.byref(c), ctypes.byref(o), 4096, n.value - 1, None) == WORKSPACE


def _cov(**kw):
    io = _lib.nrx_cov_space_io()
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols, io.num_rx_ant = 2, 2, 24, 14, 4
    io.h = io.acc = 4096
    for k, v in kw.items():
        setattr(io, k, v)
    return io


@pytest.mark.parametrize("kw,code,word", [
    (dict(h=None), INVALID_ARG, b"null"), (dict(acc=None), INVALID_ARG, b"null"),
    (dict(num_symbols=13), SHAPE, b"num_symbols"), (dict(batch=0), SHAPE, b"batch"), (dict(batch=65536), SHAPE, b"batch"),
    (dict(num_tx=0), SHAPE, b"num_tx"), (dict(num_tx=17), SHAPE, b"num_tx"),
    (dict(num_rx_ant=0), SHAPE, b"num_rx_ant"), (dict(num_rx_ant=17), SHAPE, b"num_rx_ant"),
    (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"), (dict(num_subcarriers=3301), SHAPE, b"num_subcarriers"),
])
def test_cov_space_argument_checks(lib, kw, code, word):
    io = _cov(**kw)
    n = ctypes.c_size_t(1 << 30)
    assert lib.nrx_cov_space_accumulate(ctypes.byref(io), 4096, n, None) == code
    assert word in lib.nrx_last_error()
    assert lib.nrx_cov_space_workspace_size(ctypes.byref(io), ctypes.byref(n)) == code


def test_cov_space_workspace(lib):
    io, n = _cov(), ctypes.c_size_t()
    assert lib.nrx_cov_space_workspace_size(ctypes.byref(io), ctypes.byref(n)) == OK
    assert n.value == 256 * 4 * 4 * 16             # 256 partials of A x A complex doubles
    assert lib.nrx_cov_space_workspace_size(ctypes.byref(io), None) == INVALID_ARG
    assert lib.nrx_cov_space_workspace_size(None, ctypes.byref(n)) == INVALID_ARG
    assert lib.nrx_cov_space_accumulate(None, 4096, 1 << 20, None) == INVALID_ARG
    assert lib.nrx_cov_space_accumulate(ctypes.byref(io), None, n, None) == INVALID_ARG
    assert lib.nrx_cov_space_accumulate(ctypes.byref(io), 4096, n.value - 1, None) == WORKSPACE
    assert b"workspace" in lib.nrx_last_error()
