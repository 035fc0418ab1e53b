"""Closed forms of the numpy reference of the soft-output metrics (tests/softmetrics_ref.py) and of
the host-side derivations (neural_rx_amd/softmetrics.py: derive, ebno_at_rate).  No GPU."""
import numpy as np
import pytest

from neural_rx_amd import softmetrics as SM
from tests import softmetrics_ref as R

DMRS = (2, 11)
SCALES = (0.5, 1.0, 2.0)


def _case(seed=0, H=1, B=3, U=2, F=5, bs=4, mcs_bits=(4,)):
    rng = np.random.default_rng(seed)
    llr = (rng.standard_normal((H, B, U, F, 14, bs)) * 8).astype(np.float32)
    bits = rng.integers(0, 2, (B, U, F, 14, bs)).astype(np.uint8)
    active = np.ones((B, U), np.float32)
    mcs = rng.integers(0, len(mcs_bits), (B, U)).astype(np.uint8)
    return llr, bits, active, mcs


def test_zero_llrs_give_bmi_zero_exactly():
    llr, bits, active, mcs = _case()
    loss, cnt, nonf = R.llr_stats(np.zeros_like(llr), bits, active, mcs, (4,), DMRS, SCALES)
    assert np.all(cnt[:, 0, :4] == 3 * 5 * 12) and np.all(cnt[:, 0, 4:] == 0) and not nonf.any()
    assert np.all(R.bmi_cells(loss, cnt)[0, :4] == 0.0)
    res = SM.derive(loss, cnt, nonf, (4,), SCALES)
    assert res.bmi == [0.0] and res.gmi == [0.0]


def test_confident_llrs_right_and_wrong():
    llr, bits, active, mcs = _case()
    right = ((2.0 * bits - 1.0) * 1e4).astype(np.float32)[None]
    loss, cnt, nonf = R.llr_stats(right, bits, active, mcs, (4,), DMRS, (1.0,))
    assert np.all(R.bmi_cells(loss, cnt)[0, :4, 0] == 1.0)
    loss, cnt, nonf = R.llr_stats(-right, bits, active, mcs, (4,), DMRS, (1.0,))
    # every bit costs 1e4 / ln 2 = 14426.950408889634 bits, so the BMI is 1 - 14426.95...
    np.testing.assert_allclose(loss[:, 0, :4, 0] / cnt[:, 0, :4], 14426.950408889634, rtol=1e-15)
    np.testing.assert_allclose(R.bmi_cells(loss, cnt)[0, :4, 0], 1.0 - 14426.950408889634, rtol=1e-15)


def test_doubling_the_llrs_is_scale_two():
    llr, bits, active, mcs = _case(1)
    a, cnt, _ = R.llr_stats(llr, bits, active, mcs, (4,), DMRS, (2.0, 4.0))
    b, cnt2, _ = R.llr_stats(2 * llr, bits, active, mcs, (4,), DMRS, (1.0, 2.0))
    assert np.array_equal(cnt, cnt2)
    np.testing.assert_array_equal(a, b)     # a power of two: the same float64 products


def test_masks_exclude_and_values_do_not():
    llr, bits, active, mcs = _case(2, H=1, U=3, bs=6, mcs_bits=(2, 4, 6))
    active[0, 1] = 0
    base = R.llr_stats(llr, bits, active, mcs, (2, 4, 6), DMRS, SCALES)
    l2, b2 = llr.copy(), bits.copy()
    l2[0, 0, 1] = 1e9                         # an inactive user
    l2[:, :, :, :, list(DMRS)] = np.nan       # DMRS symbols
    b2[:, :, :, list(DMRS)] ^= 1
    for b in range(3):
        for u in range(3):
            nb = (2, 4, 6)[mcs[b, u]]
            l2[0, b, u, :, :, nb:] = -77.0    # k >= m
            b2[b, u, :, :, nb:] = 1
    again = R.llr_stats(l2, b2, active, mcs, (2, 4, 6), DMRS, SCALES)
    for x, y in zip(base, again):
        np.testing.assert_array_equal(x, y)
    # a zero LLR inside the set counts: BMI contribution 0, count 1
    l3 = llr.copy()
    l3[0, 1, 0, 0, 0, 0] = 0.0
    z = R.llr_stats(l3, bits, active, mcs, (2, 4, 6), DMRS, SCALES)
    assert np.array_equal(z[1], base[1])


def test_heads_follow_the_mcs():
    llr, bits, active, mcs = _case(3, H=2, bs=4, mcs_bits=(2, 4))
    loss, cnt, _ = R.llr_stats(llr, bits, active, mcs, (2, 4), DMRS, (1.0,))
    for m in range(2):
        pick = np.where(mcs == m, 1.0, 0.0).astype(np.float32)
        lo, cn, _ = R.llr_stats(llr[m:m + 1], bits, active * pick, np.full_like(mcs, m), (2, 4), DMRS, (1.0,))
        np.testing.assert_array_equal(lo[:, m], loss[:, m])
        np.testing.assert_array_equal(cn[:, m], cnt[:, m])


def test_nonfinite_llrs_are_counted_apart():
    llr, bits, active, mcs = _case(4)
    base = R.llr_stats(llr, bits, active, mcs, (4,), DMRS, SCALES)
    bad = llr.copy()
    bad[0, 0, 0, 0, 0, 0] = np.nan
    bad[0, 0, 0, 1, 0, 1] = np.inf
    bad[0, 1, 1, 2, 3, 1] = -np.inf
    bad[0, 1, 1, 2, 2, 1] = np.nan            # a DMRS symbol: not in the set
    loss, cnt, nonf = R.llr_stats(bad, bits, active, mcs, (4,), DMRS, SCALES)
    assert nonf.sum() == 3 and nonf[0, 0, 0] == 1 and nonf[0, 0, 1] == 1 and nonf[1, 0, 1] == 1
    assert cnt.sum() == base[1].sum() - 3
    assert np.all(np.isfinite(loss))
    zeroed = np.where(np.isfinite(bad), bad, 0.0).astype(np.float32)
    lz, cz, _ = R.llr_stats(zeroed, bits, active, mcs, (4,), DMRS, SCALES)
    # a zero LLR costs exactly 1 bit at every scale: the only difference to dropping the entry
    np.testing.assert_allclose(lz.sum((0, 1, 2)) - loss.sum((0, 1, 2)), 3.0, atol=1e-9)


def test_nmse_reference():
    rng = np.random.default_rng(5)
    h = rng.standard_normal((3, 2, 5, 14, 4)).astype(np.float32)
    he = (h + 0.5).astype(np.float32)
    active = np.array([[1, 1], [0, 1], [1, 1]], np.float32)
    err, ref, items = R.chest_nmse(he, h, active)
    assert items.tolist() == [2, 3]
    d = he.astype(np.float64) - h
    np.testing.assert_allclose(err, [(d[[0, 2], 0] ** 2).sum(), (d[:, 1] ** 2).sum()], rtol=1e-14)
    e2, r2, _ = R.chest_nmse(he, h, active, symbol_mask=(1 << 2) | (1 << 11))
    np.testing.assert_allclose(e2[1], (d[:, 1][:, :, [2, 11]] ** 2).sum(), rtol=1e-14)
    assert R.chest_nmse(h, h, active)[0].tolist() == [0.0, 0.0]
    res = SM.derive(np.zeros((2, 1, 8, 1)), np.zeros((2, 1, 8), np.int64), np.zeros((2, 1, 8), np.int64), (4,), (1.0,),
                    err, ref, items)
    assert res.nmse == pytest.approx(err.sum() / ref.sum(), rel=1e-15) and res.channel_items == 5
    assert np.isnan(res.bmi[0]) and res.as_dict()["bmi"] == [None]
    assert SM.derive(np.zeros((2, 1, 8, 1)), np.zeros((2, 1, 8), np.int64), np.zeros((2, 1, 8), np.int64), (4,),
                     (1.0,)).nmse is None


def test_derive_means_and_gmi():
    """bmi[m] is the count-weighted mean over k < bits[m] at the scale nearest 1; gmi its best scale"""
    llr, bits, active, mcs = _case(6, U=2, bs=4, mcs_bits=(2, 4))
    over = (llr * 3).astype(np.float32)                    # over-confident: the best scale is below 1
    scales = (0.25, 0.354, 0.5, 0.707, 1.1, 2.0)
    loss, cnt, nonf = R.llr_stats(over, bits, active, mcs, (2, 4), DMRS, scales)
    res = SM.derive(loss, cnt, nonf, (2, 4), scales)
    cells = R.bmi_cells(loss, cnt)
    for m, nb in enumerate((2, 4)):
        w = cnt.sum(0)[m, :nb]
        per_s = (cells[m, :nb] * w[:, None]).sum(0) / w.sum()
        assert res.bmi[m] == pytest.approx(per_s[4], abs=1e-12)
        assert res.gmi[m] == pytest.approx(per_s.max(), abs=1e-12)
        assert res.gmi_scale[m] == scales[int(per_s.argmax())]
        assert res.gmi[m] >= res.bmi[m]
    np.testing.assert_allclose(np.asarray(res.bmi_bits, float)[0, :2], cells[0, :2], atol=1e-15)
    # per-user variants keep u
    one = SM.derive(loss[:1], cnt[:1], nonf[:1], (2, 4), scales)
    assert res.bmi_user[0] == pytest.approx(one.bmi, abs=1e-15)


def test_ebno_at_rate():
    curve = list(zip([0.0, 2.0, 4.0, 6.0], [0.2, 0.4, 0.8, 0.9]))
    assert SM.ebno_at_rate(curve, 0.6) == pytest.approx(3.0)
    assert SM.ebno_at_rate(curve, 0.95) is None                 # never reached
    assert SM.ebno_at_rate(curve, 0.1) is None                  # never below: no crossing from below
    assert SM.ebno_at_rate(curve, 0.4) == 2.0                   # at a sample
    assert SM.ebno_at_rate(curve, 0.2) == 0.0                   # at the first sample
    dip = list(zip([0.0, 1.0, 2.0, 3.0, 4.0], [0.7, 0.3, 0.5, 0.2, 0.9]))
    assert SM.ebno_at_rate(dip, 0.4) == pytest.approx(1.5)      # the first upward crossing
    assert SM.ebno_at_rate([], 0.5) is None


def test_accumulator_argument_checks():
    with pytest.raises(ValueError):
        SM.SoftAccumulator(2, (4,), scales=(), device=None)
    with pytest.raises(ValueError):
        SM.SoftAccumulator(2, (4,), scales=(1.0, -1.0), device=None)
    with pytest.raises(ValueError):
        SM.SoftAccumulator(2, (4,), scales=(float("inf"),), device=None)
    with pytest.raises(ValueError):
        SM.SoftAccumulator(2, (9,), device=None)
    acc = SM.SoftAccumulator(2, (2, 4), device=None)
    assert tuple(acc.loss.shape) == (2, 2, 8, 9) and tuple(acc.cnt.shape) == (2, 2, 8)
    with pytest.raises(RuntimeError):
        acc.add_llr(None, None, None, None, DMRS)
