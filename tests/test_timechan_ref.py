"""Identities of the time-domain channel's numpy statement (tests/timechan_ref.py) itself, on the host:
N = 64, F = 48, cyclic prefix (6, 4, ..., 4), fs = N scs."""
import functools

import numpy as np

from oracle import synth_ref as S
from tests import ofdm_ref as O
from tests import timechan_ref as R

B, U, F, A, N = 3, 2, 48, 2, 64
CP = tuple([6] + [4] * 13)
SCS = 30e3
FS = N * SCS
LS = sum(CP) + 14 * N


def _spec(**kw):
    base = dict(batch=B, num_tx=U, num_subcarriers=F, num_rx_ant=A, mcs_bits=(2, 4), mcs_of_user=(-1, 1), num_taps=3,
                num_sinusoids=4, max_delay_s=300e-9, max_doppler_hz=0.0, subcarrier_spacing=SCS, no=0.02, seed=53,
                slot_offset=7)
    base.update(kw)
    return S.GenSpec(**base)


@functools.lru_cache(maxsize=None)
def _plain():
    return S.generate(_spec())


def _hx(o):
    return np.einsum("buaft,buft->baft", o.h_c, o.base.x)


def test_an_integer_delay_without_doppler_shifts_and_scales():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 1, 200)) + 1j * rng.standard_normal((2, 1, 200))
    g0 = (rng.standard_normal((2, 1, 3, 1, 1)) + 1j * rng.standard_normal((2, 1, 3, 1, 1)))
    for k in (0, 1, 5):
        tau = np.full((2, 1, 1), k / FS)
        r = R.time_channel(x, tau, g0, np.zeros(g0.shape), FS, n0=17, l_min=-3, l_max=5)
        want = np.zeros((2, 3, 200), np.complex128)
        want[:, :, k:] = g0[:, 0, :, 0, 0, None] * x[:, 0, None, :200 - k]
        err = np.abs(r - want).max()
        print("delay", k, "error", err)
        assert err <= 1e-13 * np.abs(want).max()


def test_static_paths_inside_the_prefix_are_the_diagonal_channel():
    """l_max <= cp - ta and ta >= -l_min: no inter-symbol and no inter-carrier interference, so the noise-free
    demodulated grid is sum_u h o x with the statement's h.  Both sides are f64 sums of < 10^3 terms."""
    for l_min, l_max, ta in ((0, 4, 0), (-2, 2, 2), (-1, 2, 1)):
        o = R.generate(_spec(), N, CP, l_min, l_max, ta, base=_plain())
        want = _hx(o)
        err = np.abs(o.y_free - want).max()
        print("taps", l_min, l_max, "advance", ta, "error", err, "scale", np.abs(want).max())
        assert err <= 1e-12 * np.abs(want).max()


def test_a_delay_beyond_the_prefix_or_a_doppler_leaves_a_residual():
    cases = {"delay beyond the prefix": (_spec(max_delay_s=12 / FS), -2, 18),
             "doppler": (_spec(max_doppler_hz=20e3), 0, 4)}
    for name, (s, l_min, l_max) in cases.items():
        o = R.generate(s, N, CP, l_min, l_max, 2 if l_min else 0)
        want = _hx(o)
        res = np.abs(o.y_free - want).max()
        print(name, "residual", res, "scale", np.abs(want).max())
        assert res > 1e-3 * np.abs(want).max()


def test_without_doppler_h_approaches_the_plain_generators_as_the_span_grows():
    plain = _plain()
    hp = np.moveaxis(plain.h[..., :A].astype(np.float64) + 1j * plain.h[..., A:].astype(np.float64), -1, 2)
    gap = {}
    for l_min, l_max in ((-3, 5), (-16, 24)):
        tau, g0, fd = R.channel_draws(_spec(), N)
        h = R.effective_h(tau, g0, fd, N, CP, F, FS, CP[0], l_min, l_max, 0)
        gap[(l_min, l_max)] = np.abs(h - hp).max() / np.abs(hp).max()
    print("relative gap to the plain h:", gap)
    assert gap[(-16, 24)] < gap[(-3, 5)] < 0.2


def test_the_generators_conventions():
    """the samples are modulate(x), n0 = cp[0], bits / mcs / active are the plain run's, the noise is its noise"""
    o = R.generate(_spec(), N, CP, -6, -1, 0, base=_plain())
    assert o.r.shape == (B, A, LS) and o.xs.shape == (B, U, LS)
    np.testing.assert_array_equal(o.xs, O.modulate(_plain().x, N, CP))
    assert R.resolve_l_max(-1, [300e-9], FS) == 7 and R.resolve_l_max(9, [1.0], FS) == 9
    hp = _plain().h                                     # f32, so the plain run's noise is known to about 1e-7 |h x|
    hx = np.einsum("bufta,buft->bfta", hp[..., :A].astype(np.float64) + 1j * hp[..., A:].astype(np.float64), _plain().x)
    np.testing.assert_allclose(np.moveaxis(R.noise(_spec()), 1, -1), np.moveaxis(_plain().y_c, 1, -1) - hx, atol=1e-6)


def test_float64_against_longdouble():
    rng = np.random.default_rng(2)
    sh = (2, 2, 2, 3, 4)
    x = rng.standard_normal((2, 2, 300)) + 1j * rng.standard_normal((2, 2, 300))
    tau = rng.uniform(0, 3 / FS, (2, 2, 3))
    g0 = rng.standard_normal(sh) + 1j * rng.standard_normal(sh)
    fd = rng.uniform(-20e3, 20e3, sh)
    r = R.time_channel(x, tau, g0, fd, FS, 6, -3, 5)
    rl = R.time_channel(x, tau, g0, fd, FS, 6, -3, 5, real=np.longdouble)
    e = float(np.abs(r - rl).max() / np.abs(rl).max())
    print("f64 statement against longdouble:", e)
    assert rl.dtype == np.clongdouble and e < 1e-13
