"""The numpy statement of the channel-impulse-response replay (tests/cir_ref.py) against itself and against
``oracle/synth_ref.py``."""
import numpy as np

from oracle import synth_ref as S
from tests import cir_ref as R


def _spec(**kw):
    base = dict(batch=3, num_tx=2, num_subcarriers=24, num_rx_ant=3, mcs_bits=(2, 4), mcs_of_user=(-1, 1), seed=91,
                slot_offset=5, no=0.02)
    base.update(kw)
    return S.GenSpec(**base)


def _dataset(E, A, L, Ta, seed=0, max_delay=400e-9):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((E, A, L, Ta)) + 1j * rng.standard_normal((E, A, L, Ta))) / np.sqrt(2 * L)
    return R.round_f32(a, rng.uniform(0, max_delay, (E, L)))


def test_one_path_without_delay_is_flat_and_equal_to_a():
    a = np.array([0.3 - 0.4j, -1.0 + 0.25j, 2.0j]).reshape(1, 3, 1, 1)
    H = R.channel(a, np.zeros((1, 1)), np.zeros((2, 2), np.int64), 24, 30e3, f_offset=-12.0)
    assert H.shape == (2, 2, 3, 24, 14)
    np.testing.assert_array_equal(H, np.broadcast_to(a.reshape(1, 1, 3, 1, 1), H.shape))
    # one coefficient per symbol: the symbol axis follows a
    a14 = a * np.exp(1j * np.arange(14))[None, None, None, :]
    H = R.channel(a14, np.zeros((1, 1)), np.zeros((1, 1), np.int64), 5, 30e3)
    np.testing.assert_array_equal(H[0, 0], np.broadcast_to(a14[0, :, 0, None, :], (3, 5, 14)))


def test_f_offset_shifts_only_the_per_path_phase():
    a, tau = _dataset(2, 3, 5, 14)
    e = np.array([[0, 1]])
    scs, off = 30e3, -12.0
    H0 = R.channel(a, tau, e, 24, scs)
    H1 = R.channel(a, tau, e, 24, scs, f_offset=off)
    rot = a * np.exp(-2j * np.pi * off * scs * tau)[:, None, :, None]
    np.testing.assert_allclose(H1, R.channel(rot, tau, e, 24, scs), rtol=0, atol=1e-12 * np.abs(H0).max())
    # a shift by whole subcarriers moves the grid: H1[f] = H0[f + off] where both exist
    H2 = R.channel(a, tau, e, 24, scs, f_offset=3.0)
    np.testing.assert_allclose(H2[..., :21, :], H0[..., 3:, :], rtol=0, atol=1e-12 * np.abs(H0).max())
    assert np.abs(H1 - H0).max() > 1e-3


def test_normalize_gives_unit_mean_energy_and_zeros_for_an_empty_example():
    a, tau = _dataset(3, 3, 7, 1)
    a[1] = 0
    e = np.array([[0, 1], [2, -1]])
    H = R.channel(a, tau, e, 24, 30e3, f_offset=-12.0, normalize=True)
    c = np.mean(np.abs(H) ** 2, axis=(2, 3, 4))
    np.testing.assert_allclose(c[[0, 1], [0, 0]], 1.0, rtol=1e-13)
    assert (H[0, 1] == 0).all() and (H[1, 1] == 0).all()
    raw = R.channel(a, tau, e, 24, 30e3, f_offset=-12.0)
    np.testing.assert_allclose(H[0, 0], raw[0, 0] / np.sqrt(np.mean(np.abs(raw[0, 0]) ** 2)), rtol=1e-14)


def test_selection_is_reproducible_and_trajectory_keeps_the_user():
    s = _spec(batch=64, num_tx=3)
    for sel in (R.SELECT_RANDOM, R.SELECT_TRAJECTORY):
        e = R.select_examples(s, 17, sel)
        np.testing.assert_array_equal(e, R.select_examples(s, 17, sel))
        assert e.min() >= 0 and e.max() < 17
        # a split of the slots selects the same examples
        lo = R.select_examples(_spec(batch=40, num_tx=3), 17, sel)
        hi = R.select_examples(_spec(batch=24, num_tx=3, slot_offset=s.slot_offset + 40), 17, sel)
        np.testing.assert_array_equal(np.concatenate([lo, hi]), e)
        assert not np.array_equal(e, R.select_examples(_spec(batch=64, num_tx=3, seed=92), 17, sel))
    w = S.draw(s.seed, s.slot_offset + np.arange(64)[:, None], R.STREAM_CIR, np.arange(3)[None, :])[0].astype(np.int64)
    np.testing.assert_array_equal(R.select_examples(s, 17, R.SELECT_RANDOM), w % 17)
    t = R.select_examples(s, 17, R.SELECT_TRAJECTORY)               # n = 5: examples 0..14
    np.testing.assert_array_equal(t % 3, np.broadcast_to(np.arange(3), t.shape))
    np.testing.assert_array_equal(t, 3 * (w % 5) + np.arange(3))
    assert t.max() < 15 and len(np.unique(t[:, 0])) == 5
    # E = 7, U = 2: n = 3
    t = R.select_examples(_spec(batch=64), 7, R.SELECT_TRAJECTORY)
    assert set(np.unique(t[:, 0])) == {0, 2, 4} and set(np.unique(t[:, 1])) == {1, 3, 5}
    idx = np.array([[0, -1], [7, 6], [3, 3]])
    np.testing.assert_array_equal(R.select_examples(_spec(), 7, R.SELECT_INDEX, idx), [[0, -1], [-1, 6], [3, 3]])


def test_replaying_the_oracles_taps_reproduces_the_oracle():
    s = _spec()
    o = S.generate(s)
    gt, tau = R.oracle_taps(s)
    a, t, index = R.as_dataset(gt, tau)
    out, H, e = R.generate(s, a, t, R.SELECT_INDEX, index, normalize=False, f_offset=0.0, base=o)
    np.testing.assert_array_equal(e, index)
    A = s.num_rx_ant
    h = o.h[..., :A].astype(np.float64) + 1j * o.h[..., A:].astype(np.float64)            # [B, U, F, T, A], f32
    scale = np.abs(H).max()
    assert np.abs(np.moveaxis(H, 2, -1) - h).max() <= 2.0 ** -24 * scale                    # the oracle's h is rounded
    assert np.abs(out.y_c - o.y_c).max() <= 1e-12 * np.abs(o.y_c).max()
    # the unrounded channel through the noise-free part of y_c: 1e-12 relative
    hx = np.einsum("buaft,buft->baft", H, o.x)
    assert np.abs((o.y_c - R.noise(s)) - hx).max() <= 1e-12 * np.abs(hx).max()
    # the rounded outputs: one float32 ulp at the most (a sum in another order can round the other way)
    for k in ("y", "h", "h_hat"):
        ref = getattr(o, k).astype(np.float64)
        assert np.abs(getattr(out, k) - ref).max() <= 2.0 ** -23 * np.abs(ref).max(), k
    for k in ("bits", "mcs", "active"):
        np.testing.assert_array_equal(getattr(out, k), getattr(o, k))


def test_zero_channel_user_leaves_no_trace_in_y():
    s = _spec()
    a, tau = _dataset(4, 3, 6, 14)
    full, _, _ = R.generate(s, a, tau, R.SELECT_INDEX, np.array([[0, 1], [2, 3], [1, 0]]))
    part, H, _ = R.generate(s, a, tau, R.SELECT_INDEX, np.array([[0, -1], [2, 3], [4, 0]]))
    assert (H[0, 1] == 0).all() and (H[2, 0] == 0).all()
    np.testing.assert_array_equal(part.y[1], full.y[1])
    only0 = np.einsum("aft,ft->aft", H[0, 0], part.x[0, 0]) + R.noise(s)[0]
    np.testing.assert_array_equal(part.y[0], R.to_ch(only0))
