"""tests/ofdm_ref.py, the numpy statement of nrx_ofdm_modulate / nrx_ofdm_demodulate and of the generator's
time-domain stage, pinned on the CPU: against itself (round trip), against a line-by-line transcription of the
reference's two ``call`` methods (utils/siona_tf.py:4452-4470, 4577-4643, unitary fft / ifft of 4331-4402), and
against the closed forms the stage is documented with."""
import numpy as np
import pytest

from tests import ofdm_ref as O

CP = [6] + [4] * 13          # non-uniform: the first symbol's prefix is longer, as in NR
EPS = 2.0 ** -52


def _grid(shape, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


@pytest.mark.parametrize("N,F,first_bin", [(64, 48, -1), (64, 25, -1), (64, 64, 0), (128, 48, 0), (128, 25, 103)])
@pytest.mark.parametrize("ta", [0, 1, 4])
def test_round_trip_to_f64_rounding(N, F, first_bin, ta):
    g = _grid((2, 3, F, 14), N + F)
    smp = O.modulate(g, N, CP, first_bin, L=sum(CP) + 14 * N + 5)
    assert smp.shape == (2, 3, sum(CP) + 14 * N + 5) and not smp[..., -5:].any()
    back = O.demodulate(smp, N, CP, F, 14, first_bin, timing_advance=ta)
    err = np.abs(back - g).max() / np.abs(g).max()
    assert err <= 8 * EPS * np.log2(N), err


def test_unitary_and_sample_power():
    """energy in = energy out per symbol; the unit-energy grid gives mean sample power F / N"""
    N, F = 64, 48
    g = _grid((4, 1, F, 14), 3)
    smp = O.modulate(g, N, 0)
    np.testing.assert_allclose((np.abs(smp) ** 2).sum(), (np.abs(g) ** 2).sum(), rtol=1e-12)
    assert abs((np.abs(smp) ** 2).mean() / (np.abs(g) ** 2).mean() - F / N) < 1e-12


# ---- the reference's layers, transcribed: tf.signal.* -> np.fft.*, tf.concat / reshape -> numpy's


def _ref_fft(x):
    return (1 / np.sqrt(x.shape[-1])) * np.fft.fft(x)


def _ref_ifft(x):
    return np.sqrt(x.shape[-1]) * np.fft.ifft(x)


def _ref_modulator_call(inputs, cyclic_prefix_length):
    """inputs [..., num_ofdm_symbols, fft_size]"""
    inputs = np.fft.ifftshift(inputs, axes=-1)
    x = _ref_ifft(inputs)
    cp = x[..., inputs.shape[-1] - cyclic_prefix_length:]
    x = np.concatenate([cp, x], -1)
    return x.reshape(x.shape[:-2] + (-1,))


def _ref_demodulator_call(inputs, fft_size, l_min, cyclic_prefix_length):
    tmp = -2 * np.pi * float(l_min) / float(fft_size) * np.arange(fft_size, dtype=np.float64)
    phase_compensation = np.exp(1j * tmp)
    rest = np.mod(inputs.shape[-1], fft_size + cyclic_prefix_length)
    num_ofdm_symbols = (inputs.shape[-1] - rest) // (fft_size + cyclic_prefix_length)
    inputs = inputs if rest == 0 else inputs[..., :-rest]
    x = inputs.reshape(inputs.shape[:-1] + (num_ofdm_symbols, fft_size + cyclic_prefix_length))
    x = x[..., cyclic_prefix_length:]
    x = _ref_fft(x)
    x = x * phase_compensation
    return np.fft.fftshift(x, axes=-1)


@pytest.mark.parametrize("N,cp", [(64, 4), (64, 0), (128, 9), (256, 18)])
def test_modulator_is_the_references_at_full_band(N, cp):
    g = _grid((2, 3, N, 14), N + cp)
    ours = O.modulate(g, N, cp, first_bin=0)
    theirs = _ref_modulator_call(np.swapaxes(g, -1, -2), cp)
    assert np.abs(ours - theirs).max() <= 8 * EPS * np.log2(N) * np.abs(theirs).max()


@pytest.mark.parametrize("N,cp,l_min,rest", [(64, 4, 0, 0), (64, 4, -3, 7), (64, 4, -4, 0), (128, 9, -9, 26)])
def test_demodulator_is_the_references_at_full_band(N, cp, l_min, rest):
    """a sequence that already starts at l_min: the reference cuts it from its first sample on, which is our
    window start cp - timing_advance shifted by an offset of +timing_advance"""
    rng = np.random.default_rng(N + cp - l_min)
    L = 14 * (N + cp) + rest
    smp = rng.standard_normal((2, 3, L)) + 1j * rng.standard_normal((2, 3, L))
    theirs = np.swapaxes(_ref_demodulator_call(smp, N, l_min, cp), -1, -2)
    ours = O.demodulate(smp, N, cp, N, 14, first_bin=0, timing_advance=-l_min, offset=-l_min)
    assert np.abs(ours - theirs).max() <= 8 * EPS * np.log2(N) * np.abs(theirs).max()
    # and the timing advance itself: the same grid from windows that start -l_min samples early in the prefix
    g = _grid((2, 3, N, 14), 5)
    tx = O.modulate(g, N, cp, first_bin=0)
    back = O.demodulate(tx, N, cp, N, 14, first_bin=0, timing_advance=-l_min)
    assert np.abs(back - g).max() <= 8 * EPS * np.log2(N) * np.abs(g).max()


def test_a_delay_inside_the_prefix_is_a_ramp_and_one_beyond_is_not():
    N, F = 64, 48
    g = _grid((1, 1, F, 14), 9)
    smp = O.modulate(g, N, CP)
    for d in (0, 1, 4):
        out = O.demodulate(smp, N, CP, F, 14, offset=-d)
        want = g * O.delay_ramp(F, N, d)[:, None]
        # symbol 0 has nothing before it but its own prefix, 6 long; every later symbol's prefix is 4
        assert np.abs(out - want).max() <= 64 * EPS, (d, np.abs(out - want).max())
    out = O.demodulate(smp, N, CP, F, 14, offset=-5)
    err = np.abs(out - g * O.delay_ramp(F, N, 5)[:, None])
    assert err[..., 0].max() <= 64 * EPS          # the longer first prefix still covers 5
    assert err[..., 1:].max() > 0.1               # inter-symbol interference everywhere else


def test_tx_stage_is_modulate_impair_demodulate():
    N, F = 64, 48
    x = _grid((3, 2, F, 14), 11)
    np.testing.assert_allclose(O.tx_stage(x, N, CP, (0, 0)), x, atol=64 * EPS)
    out = O.tx_stage(x, N, CP, (0, 3))
    np.testing.assert_allclose(out[:, 0], x[:, 0], atol=64 * EPS)
    np.testing.assert_allclose(out[:, 1], x[:, 1] * O.delay_ramp(F, N, 3)[:, None], atol=64 * EPS)
    pa = O.tx_stage(x, N, CP, (0, 0), pa_ibo_db=3.0)
    assert 0.01 < np.abs(pa - x).max() < 1.0      # a compression, not a different signal


def test_rapp_limits():
    rng = np.random.default_rng(2)
    v = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)) * 3.0
    for p in (0.5, 2.0, 10.0):
        for asat in (0.5, 1.0, 2.0):
            out = O.rapp(v, asat, p)
            # strictly below asat in exact arithmetic; deep in saturation the f64 quotient rounds onto it
            assert np.abs(out).max() <= asat * (1 + 4 * EPS)
            assert np.abs(O.rapp(v / 8, asat, p)).max() < asat
            np.testing.assert_allclose(np.angle(out), np.angle(v), atol=1e-12)     # AM/AM only
            assert np.all(np.abs(out) <= np.abs(v))
    vmax = np.abs(v).max()
    for asat in (1e2, 1e3, 1e6):      # the identity as asat grows: 1 - g <= (|v| / asat)^(2p) / (2p), first order
        assert np.abs(O.rapp(v, asat, 2.0) - v).max() <= ((vmax / asat) ** 4 / 4 + 2 * EPS) * vmax
    assert O.rapp(v, 0.0, 2.0) is v and O.rapp(v, -1.0, 2.0) is v
    assert O.rapp(v.astype(np.complex64), 1.0, 2.0).dtype == np.complex64


def test_layout_helpers_and_numerology():
    g = _grid((2, 3, 5, 14), 4)
    y = O.to_cgnn(g)
    assert y.shape == (2, 5, 14, 6) and y[1, 4, 13, 2] == g[1, 2, 4, 13].real and y[1, 4, 13, 5] == g[1, 2, 4, 13].imag
    np.testing.assert_array_equal(O.from_cgnn(y), g)
    assert O.default_cp(4096) == 288 and O.default_cp(64) == 4 and O.default_cp(128) == 9
    assert list(O.bins(4, 64, -1)) == [62, 63, 0, 1] and list(O.bins(3, 64, 0)) == [32, 33, 34]
    assert list(O.bins(25, 64, -1)[:2]) == [(32 - 12 - 32) % 64, (32 - 12 - 32) % 64 + 1]
    assert abs(O.pa_asat(48, 64, 0.0) ** 2 - 0.75) < 1e-15
