"""The soft-metric kernels (``nrx_llr_stats``, ``nrx_chest_nmse``) through ``SoftAccumulator``
against the float64 numpy reference of tests/softmetrics_ref.py (needs an MI355X).

Inputs.  LLRs ``randn * 8``; a fixed 2 % of the entries (a seeded choice) are replaced, round-robin,
by 0, +-1e-30, +-87, +-89, +-1e4, NaN, +inf and -inf; random bits.  FS = the strip of
``softmetrics.STRIP_SUBCARRIERS`` subcarriers of one work item.

    S1  H 1  B 3  U 2   F 12         stride 4  m 4                 the bench shape's row width
    S1a as S1 with one scale                                        S = 1
    S2  H 1  B 2  U 3   F 13         stride 6  MCS drawn of 2/4/6  odd F, partial wave, ragged m, user 1 of
                                                                    slot 0 inactive, one DMRS symbol
    S3  H 2  B 4  U 2   F 12         stride 4  bits (2, 4)         head = MCS
    S4  H 1  B 1  U 1   F 2 FS + 5   stride 8  m 6                 several strips per item, a strip tail
    S5  H 1  B 5  U 16  F 12         stride 2  m 2                 U at its limit
    S6  H 1  B 2  U 2   F FS + 1     stride 7  m 6  16 scales      the generic-stride rows, a one-subcarrier
                                                                    strip, S at its limit
    S7  H 1  B 6  U 2   F 12         stride 8  MCS drawn of 1..8   M at its limit (the ordered pass's rows are
                                                                    a template argument: 1, 2, 3, 4, 8)
    S8  H 1  B 6  U 2   F 12         stride 8  MCS drawn of 2/4/6/8 four MCS rows: k_llr_reduce<4>
    S9  H 1  B 300 U 2  F 12         stride 4  MCS drawn of 2/4    the ordered pass beyond its first pass: two
                                                                    chunks of 256 slots, and tiles of 81 staged
                                                                    records (7168 / (8 * 9 + 16)) of which a wave
                                                                    loads 4 per step; inactive users on both
                                                                    sides of the chunk boundary

Gates.  cnt and nonfinite equal the reference exactly.  For every cell with cnt > 0 and every scale
|bmi_gpu - bmi_ref| <= 1e-6: the linear term of the loss is exact in float64; the bounded term is
allowed 4 f32 ulps of ln 2 = 1.6e-7 nats = 2.4e-7 bits; float64 summation adds n 2^-53; 1e-6 is four
times that budget and does not depend on the size of the LLRs (hence the +-1e4 among the inputs).
The NMSE sums are held to 1e-10 relative: n 2^-53 with n < 2^17 terms, rounded up.

Figures of an MI355X run (as the tests print them): max |bmi_gpu - bmi_ref| between 2.1e-10 (S1a)
and 3.5e-9 (S7) over the cases (S8 3.3e-9, S9 7.3e-10), with cell BMIs down to -833 because of the
wrong-signed +-1e4 entries; NMSE sums within 2.3e-16 relative.
"""
import functools

import numpy as np
import pytest

from neural_rx_amd import softmetrics as SM
from tests import softmetrics_ref as R

pytestmark = pytest.mark.gpu

FS = SM.STRIP_SUBCARRIERS
SPECIALS = np.array([0.0, 1e-30, -1e-30, 87.0, -87.0, 89.0, -89.0, 1e4, -1e4, np.nan, np.inf, -np.inf], np.float32)
# name: (H, B, U, F, stride, mcs_bits, dmrs symbols, inactive (b, u) pairs, scales)
CASES = {
    "S1": (1, 3, 2, 12, 4, (4,), (2, 11), (), SM.DEFAULT_SCALES),
    "S1a": (1, 3, 2, 12, 4, (4,), (2, 11), (), (1.0,)),
    "S2": (1, 2, 3, 13, 6, (2, 4, 6), (2,), ((0, 1),), SM.DEFAULT_SCALES),
    "S3": (2, 4, 2, 12, 4, (2, 4), (2, 11), (), SM.DEFAULT_SCALES),
    "S4": (1, 1, 1, 2 * FS + 5, 8, (6,), (2, 11), (), SM.DEFAULT_SCALES),
    "S5": (1, 5, 16, 12, 2, (2,), (2, 11), (), SM.DEFAULT_SCALES),
    "S6": (1, 2, 2, FS + 1, 7, (6,), (2, 11), (), tuple(2.0 ** (0.25 * (j - 8)) for j in range(16))),
    "S7": (1, 6, 2, 12, 8, (1, 2, 3, 4, 5, 6, 7, 8), (2, 11), ((3, 0),), SM.DEFAULT_SCALES),
    "S8": (1, 6, 2, 12, 8, (2, 4, 6, 8), (2, 11), (), SM.DEFAULT_SCALES),
    "S9": (1, 300, 2, 12, 4, (2, 4), (2, 11), ((0, 1), (255, 0), (256, 0), (299, 1)), SM.DEFAULT_SCALES),
}
BMI_GATE = 1e-6


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """host inputs of a case and their reference sums, made once"""
    H, B, U, F, bs, mcs_bits, dmrs, inactive, scales = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    llr = (rng.standard_normal((H, B, U, F, 14, bs)) * 8).astype(np.float32)
    pick = np.sort(rng.choice(llr.size, llr.size // 50, replace=False))
    llr.reshape(-1)[pick] = SPECIALS[np.arange(pick.size) % SPECIALS.size]
    bits = rng.integers(0, 2, (B, U, F, 14, bs)).astype(np.uint8)
    active = np.ones((B, U), np.float32)
    for b, u in inactive:
        active[b, u] = 0
    mcs = rng.integers(0, len(mcs_bits), (B, U)).astype(np.uint8)
    ref = R.llr_stats(llr, bits, active, mcs, mcs_bits, dmrs, scales)
    for a in (llr, bits, active, mcs, *ref):
        a.setflags(write=False)
    return (llr, bits, active, mcs), ref


def _run(name, lo=None, hi=None, acc=None, shift=False):
    """one add_llr of slots [lo, hi) of a case into ``acc`` (a fresh accumulator by default)"""
    import torch
    H, B, U, F, bs, mcs_bits, dmrs, _, scales = CASES[name]
    (llr, bits, active, mcs), _ = _inputs(name)
    sl = slice(lo, hi)
    def dev(a):
        t = torch.from_numpy(np.array(a)).cuda()      # a copy: the cached inputs are read-only
        if not shift:
            return t
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")   # one element off the natural alignment
        buf[1:] = t.reshape(-1)
        return buf[1:].view(t.shape)

    acc = acc or SM.SoftAccumulator(U, mcs_bits, scales)
    acc.add_llr(dev(llr[:, sl]), dev(bits[sl]), dev(active[sl]), dev(mcs[sl]), dmrs)
    torch.cuda.synchronize()
    return acc


def _check(name, arr, ref):
    loss, cnt, nonf = ref
    assert np.array_equal(arr["cnt"], cnt), name
    assert np.array_equal(arr["nonfinite"], nonf), name
    assert cnt.sum() > 0 and nonf.sum() > 0
    got, want = R.bmi_cells(arr["loss"], arr["cnt"]), R.bmi_cells(loss, cnt)
    cells = cnt.sum(0) > 0
    d = np.abs(got - want)[cells]
    print(f"{name}: cells {int(cells.sum())}  max |bmi_gpu - bmi_ref| {d.max():.3e}  "
          f"bmi range [{want[cells].min():.4g}, {want[cells].max():.4g}]")
    assert np.all(np.isfinite(arr["loss"]))
    assert d.max() <= BMI_GATE, (name, d.max())
    assert np.all(arr["loss"][~np.broadcast_to(cells[None, ..., None], arr["loss"].shape)] == 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_llr_stats_match_the_reference(name):
    acc = _run(name)
    assert acc.items.sum().item() == 0 and acc.err.sum().item() == 0
    _check(name, acc.arrays(), _inputs(name)[1])
    # determinism: a second call on fresh accumulators is bit-identical
    again = _run(name)
    assert np.array_equal(acc.i64.cpu().numpy(), again.i64.cpu().numpy())
    assert np.array_equal(acc.f64.cpu().numpy().view(np.int64), again.f64.cpu().numpy().view(np.int64))
    # and so is the result object's BMI, within the same gate of the reference's derivation
    _, B, U, _, _, mcs_bits, _, _, scales = CASES[name]
    res, ref = acc.result(), SM.derive(*_inputs(name)[1], mcs_bits, scales)
    assert res.nonfinite == ref.nonfinite and res.nmse is None
    assert np.allclose(res.bmi, ref.bmi, rtol=0, atol=BMI_GATE, equal_nan=True)
    assert np.allclose(res.gmi, ref.gmi, rtol=0, atol=BMI_GATE, equal_nan=True)
    assert 1.0 in scales and all(g >= b for g, b in zip(res.gmi, res.bmi) if b == b)


def test_unaligned_tensors_take_the_scalar_rows():
    """the vector rows are chosen by alignment: the same values one element off give the same sums"""
    acc = _run("S1", shift=True)
    _check("S1 unaligned", acc.arrays(), _inputs("S1")[1])


def test_accumulation_and_shard_sum():
    """one call on B = 4 against two calls (slots 0-1, then 2-3) into one accumulator, and against
    the host sum of two accumulators -- the property the all-reduce relies on"""
    whole = _run("S3").arrays()
    two = _run("S3", 2, 4, acc=_run("S3", 0, 2)).arrays()
    a, b = _run("S3", 0, 2).arrays(), _run("S3", 2, 4).arrays()
    for other in (two, {k: a[k] + b[k] for k in a}):
        assert np.array_equal(other["cnt"], whole["cnt"]) and np.array_equal(other["nonfinite"], whole["nonfinite"])
        np.testing.assert_allclose(other["loss"], whole["loss"], rtol=1e-12, atol=0)
    _check("S3 in two calls", two, _inputs("S3")[1])


# ---- NMSE -------------------------------------------------------------------------------------
# name: (B, U, F, A, symbol mask, inactive pairs)
NMSE_CASES = {"N1": (3, 2, 12, 4, 0, ()), "N2": (2, 3, 13, 1, (1 << 2) | (1 << 11), ((1, 2),)),
              "N3": (2, 2, 2 * FS + 3, 3, 0b11111111111011, ())}


@functools.lru_cache(maxsize=None)
def _channels(name):
    B, U, F, A, mask, inactive = NMSE_CASES[name]
    rng = np.random.default_rng(sorted(NMSE_CASES).index(name) + 200)
    h = rng.standard_normal((B, U, F, 14, 2 * A)).astype(np.float32)
    he = (h + 1e-2 * rng.standard_normal(h.shape)).astype(np.float32)
    he[0] = h[0]                                      # one slot with a perfect estimate
    active = np.ones((B, U), np.float32)
    for b, u in inactive:
        active[b, u] = 0
    return he, h, active, R.chest_nmse(he, h, active, mask)


@pytest.mark.parametrize("name", sorted(NMSE_CASES))
@pytest.mark.parametrize("shift", [False, True])
def test_chest_nmse_matches_the_reference(name, shift):
    import torch
    B, U, F, A, mask, _ = NMSE_CASES[name]
    he, h, active, (err, ref, items) = _channels(name)

    def dev(a, off=shift):
        buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(a).reshape(-1).cuda()
        return buf[1:].view(a.shape) if off else torch.from_numpy(a).cuda()

    def run(lo, hi):
        acc = SM.SoftAccumulator(U, (4,))
        acc.add_channel(dev(he[lo:hi]), dev(h[lo:hi]), dev(active[lo:hi], False), mask)
        torch.cuda.synchronize()
        return acc

    acc, again = run(0, B), run(0, B)
    a = acc.arrays()
    assert np.array_equal(a["items"], items) and a["cnt"].sum() == 0
    print(f"{name}: max |err - err_ref| / max err_ref {np.abs(a['err'] - err).max() / err.max():.2e}  "
          f"the same for ref {np.abs(a['ref'] - ref).max() / ref.max():.2e}")
    np.testing.assert_allclose(a["err"], err, rtol=1e-10, atol=0)
    np.testing.assert_allclose(a["ref"], ref, rtol=1e-10, atol=0)
    assert np.array_equal(acc.f64.cpu().numpy().view(np.int64), again.f64.cpu().numpy().view(np.int64))
    res = acc.result()
    assert abs(res.nmse - err.sum() / ref.sum()) <= 1e-10 * res.nmse and res.channel_items == items.sum()
    assert 1e-5 < res.nmse < 2e-4                     # 1e-4 on the noisy slots, 0 on the first
    # the slot with h_est = h contributes exactly 0
    first = run(0, 1).arrays()
    assert np.all(first["err"] == 0.0) and np.all(first["ref"][active[0] > 0] > 0)
    assert np.array_equal(first["items"], (active[0] > 0).astype(np.int64))
