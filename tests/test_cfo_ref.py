"""The numpy statement of the carrier frequency offset (tests/cfo_ref.py) against its definition:
the closed-form Dirichlet-kernel product equals OFDM modulation, a rotation of the time samples and
demodulation.  Tolerance 1e-12 absolute on grids of unit-energy symbols: both sides are float64 sums
of at most 128 terms of magnitude <= 1 (N 2^-53 = 1.4e-14 each way)."""
import numpy as np
import pytest

from oracle import synth_ref as S
from tests import cfo_ref as R

SHAPES = [(24, 24), (48, 64), (36, 128)]
EPS = [0.0, 0.013, -0.2, 0.5, 1.0, 1.3]


def _grid(F, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((F, 14)) + 1j * rng.standard_normal((F, 14))) / np.sqrt(2.0)


@pytest.mark.parametrize("F,N", SHAPES)
@pytest.mark.parametrize("eps", EPS)
def test_closed_form_equals_ifft_rotate_fft(F, N, eps):
    x = _grid(F, 100 * F + N)
    assert np.abs(R.apply(x, eps, N) - R.ofdm_chain(x, eps, N)).max() <= 1e-12


@pytest.mark.parametrize("eps", EPS)
def test_full_grid_map_is_unitary(eps):
    x = _grid(24, 3)
    assert abs(np.linalg.norm(R.apply(x, eps, 24)) - np.linalg.norm(x)) <= 1e-12 * np.linalg.norm(x)
    C = R.toeplitz(24, eps, 24)
    assert np.abs(C @ C.conj().T - np.eye(24)).max() <= 1e-12


def test_one_spacing_is_an_exact_circular_shift():
    """eps = 1 with N = F: subcarrier m lands on m + 1 (mod F), bit for bit up to the symbol phasor"""
    x = _grid(24, 5)
    C = R.toeplitz(24, 1.0, 24)
    np.testing.assert_array_equal(C, np.roll(np.eye(24), 1, axis=0).astype(np.complex128))
    np.testing.assert_array_equal(C @ x, np.roll(x, 1, axis=0))


def test_zero_offset_is_the_identity():
    x = _grid(36, 7)
    np.testing.assert_array_equal(R.apply(x, 0.0, 64), x)


def test_lags_are_periodic_and_accurate_at_large_lags():
    d = np.arange(-127, 128)
    np.testing.assert_allclose(R.lags(d + 128, 0.3, 128), R.lags(d, 0.3, 128), rtol=0, atol=1e-15)
    # against the textbook formula in extended precision
    v = (d + np.longdouble(0.3))
    ref = np.exp(1j * (np.pi * 127 * v / 128).astype(np.float64)) * (np.sin(np.pi * v) / (128 * np.sin(np.pi * v / 128))).astype(np.float64)
    assert np.abs(R.lags(d, 0.3, 128) - ref).max() <= 1e-13


def test_eps_draw_uses_its_own_stream():
    s = S.GenSpec(batch=4, num_tx=3, num_subcarriers=12, num_rx_ant=2, cdm_group=(0, 1, 0), seed=9, slot_offset=2 ** 33)
    e = R.draw_eps(s, [300.0, 0.0, 600.0], constant=False)
    assert e.shape == (4, 3) and (np.abs(e[:, 0]) <= 0.01).all() and (e[:, 1] == 0).all() and (np.abs(e[:, 2]) <= 0.02).all()
    assert len(np.unique(e[:, 0])) == 4
    np.testing.assert_array_equal(R.draw_eps(s, [300.0, 0.0, 600.0], constant=True), np.tile([0.01, 0.0, 0.02], (4, 1)))
    # the slot, not the batch, decides the draw
    s2 = S.GenSpec(batch=2, num_tx=3, num_subcarriers=12, num_rx_ant=2, cdm_group=(0, 1, 0), seed=9, slot_offset=2 ** 33 + 2)
    np.testing.assert_array_equal(R.draw_eps(s2, [300.0, 0.0, 600.0], constant=False), e[2:])


def test_generate_without_offset_is_the_generator():
    s = S.GenSpec(batch=2, num_tx=2, num_subcarriers=12, num_rx_ant=2, seed=4)
    o = R.generate(s, [0.0, 0.0], h_with_phase=True)
    np.testing.assert_array_equal(o.y, o.base.y)
    np.testing.assert_array_equal(o.h_hat, o.base.h_hat)
    np.testing.assert_array_equal(o.h, o.base.h)


def test_estimator_and_rotation_on_a_pure_rotation():
    """h_hat = h0 e^{j 2 pi kappa eps t}: the estimate is eps, the nearest-DMRS rotation turns every
    symbol to its own phase, the zero-reference de-rotation removes the rotation"""
    rng = np.random.default_rng(1)
    B, U, F, A, dm = 3, 2, 12, 2, (2, 7, 11)
    eps = np.array([[0.03, -0.02], [0.0, 0.045], [-0.01, 0.02]])
    h0 = rng.standard_normal((B, U, F, 1, A)) + 1j * rng.standard_normal((B, U, F, 1, A))
    rot = np.exp(2j * np.pi * R.KAPPA * eps[:, :, None, None, None] * np.arange(14)[None, None, None, :, None])
    true = R._chan(h0 * rot)
    tref = R.nearest_symbol(dm)
    np.testing.assert_array_equal(tref, [2, 2, 2, 2, 2, 7, 7, 7, 7, 7, 11, 11, 11, 11])     # ties: the first listed
    nn = true[:, :, :, tref]
    active = np.array([[1, 1], [1, 0], [1, 1]], np.float32)
    est = R.estimate(nn, active, dm, (0, 1))
    assert est[1, 1] == 0.0
    assert np.abs((est - eps) * active).max() <= 1e-7                                       # f32 inputs
    comp = R.rotate(nn, eps, dm, R.REF_NEAREST_DMRS, +1)
    assert np.abs(comp - true).max() <= 1e-6 * np.abs(true).max()
    flat = R.rotate(true, eps, dm, R.REF_ZERO, -1)
    assert np.abs(flat - R._chan(h0 * np.ones_like(rot))).max() <= 1e-6 * np.abs(true).max()
    assert (R.estimate(nn, active, (2,), (0, 1)) == 0).all()
