"""The launch plan of every forward (``plan_forward``, csrc/nrx_dispatch.hip) over the thresholds the planner has,
without a GPU: ``nrx_debug_forward_plan`` answers for 256 CUs in 8 XCDs (the MI355X), the plan is reduced to per-kernel
profiler counts by the profiler's own rule, and the counts are held against tests/golden/forward_plans.json, which
tests/golden/make_forward_plans.py recorded from executed forwards of the library before the plan existed (launch
counts per kernel, ``CGNNEngine.profile_read``).  The golden covers 256 CUs / 8 XCDs only.

SHAPES: (topology, rx antennas, users, PRBs, slots); every one is crossed with MASKS x FUSED x NUM_IT.  At 256 CUs,
4 PRB (F = 48):

* U = 1: P16S (8-row strips, 6 per slot) fits while 6 B <= 256: B = 42 in, 43 out; P16M (16-row, 3 per slot) while
  3 B <= 256: B = 85 in, 86 out (neither tier: the 24-row tier).  Two LLR heads + ChEst (75 KB) exceed the 14-slot
  image of P16S (56 KB), so nrx_rt_var_mcs takes P16M up to 85.
* U = 2: the 24-row tier has 2 strips, items = 4 B.  Strip pairing needs items >= 2 * 256 and items % 16 == 0: B = 127
  (508) off, 128 (512) on, 130 (520, % 16 = 8) off.  A column is one item per (slot, user), items = 2 B: the one-item
  kernels and k_fwd_col need items <= 256: B = 128 in, 129 out.  k_forward needs items (4 B) >= 512: B = 127 out.
* 5 PRB (F = 60 > 48): two column strips, so the column updates need mask bit 64.
* U = 3: combine launches, combine stages in k_forward.
* 8 / 16 rx antennas (2A = 16 / 32): strip StateInit, 2A = 32 the ch32 updates.
* nrx_rt_var_mcs: two LLR heads, the strip readout.
BASELINE: the six shards of tests/test_gpu_default_paths.py at the default schedule, once each.
"""
import ctypes
import json
import os

import pytest

from neural_rx_amd import _lib
from neural_rx_amd.config import get_config, spec_from_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_plans.json")
TOPOLOGIES = ["nrx_rt", "nrx_rt_var_mcs", "nrx_large_var_mcs_64qam_masking", "nrx_large", "nrx_large_64qam"]
MASKS = [0, 1, 2, 3, 4, 8, 12, 16, 29, 31, 29 | 32, 29 | 64, 127]
FUSED = [0, 1, 2]
DEFAULT_MASK = 29
SHAPES = ([(t, 4, u, prbs, b) for t in TOPOLOGIES
           for u, prbs, b in [(1, 4, 42), (1, 4, 43), (1, 4, 85), (1, 4, 86), (2, 4, 127), (2, 4, 128), (2, 4, 129),
                              (2, 4, 130), (2, 5, 128), (3, 4, 128)]]
          + [("nrx_rt", 8, 2, 4, 128), ("nrx_rt", 16, 2, 4, 128)])
BASELINE = [("nrx_rt", 4, 1, 4, 1), ("nrx_rt", 4, 2, 4, 128), ("nrx_large", 16, 4, 132, 64),
            ("nrx_rt_var_mcs", 4, 2, 4, 128), ("nrx_large_var_mcs_64qam_masking", 4, 2, 4, 128),
            ("nrx_large_64qam", 4, 8, 273, 32)]
# nrx_debug_forward_plan: records of 16 int32.  Per chunk (b0, n, -1, path, num_init, num_it, norm_pre, gz,
# inline_combine, grid, lds, a2p, heads_x, nq, one_launch, combine launches), then per stage (b0, n, stage, kind,
# kernel id, tail, chp, one, pair, items, strips, grid, lds, order_rev, 0, 0)
REC = 16
H_NUM_INIT, H_NUM_IT, H_NORM_PRE, H_GRID = 4, 5, 6, 9
STRIP, RR, COL = 0, 1, 2
TAIL_READOUT_WB = 2
K_NORM, K_COMBINE = 0, 5


def shape_key(shape):
    return "%s a%d u%d prb%d b%d" % shape


def spec_of(shape):
    return spec_from_config(get_config(shape[0]), shape[1])


def num_its(spec):
    return sorted({1, 2, spec.num_it})


def combos(shape):
    """(num_it, fused, mask) of a SHAPES entry, in the order of its golden list"""
    return [(n, f, m) for n in num_its(spec_of(shape)) for f in FUSED for m in MASKS]


def plan(lib, shape, num_it, mask, fused, cus=256, xccs=8, precision=0):
    """[(header record, [stage records])] per slot chunk"""
    fn = lib.nrx_debug_forward_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(_lib.nrx_desc), ctypes.POINTER(_lib.nrx_shape)] + [ctypes.c_int32] * 6 + [
        ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]
    desc = _lib.make_desc(spec_of(shape))
    _, _, users, prbs, batch = shape
    sh = _lib.nrx_shape(batch, users, 12 * prbs, 14)
    cap = REC * 17 * 64
    out = (ctypes.c_int32 * cap)()
    n = fn(ctypes.byref(desc), ctypes.byref(sh), precision, num_it, mask, fused, cus, xccs, out, cap)
    assert 0 < n <= cap and n % REC == 0, (n, lib.nrx_last_error())
    recs = [list(out[i:i + REC]) for i in range(0, n, REC)]
    chunks = []
    for r in recs:
        if r[2] == -1:
            chunks.append((r, []))
        else:
            assert r[:2] == chunks[-1][0][:2] and r[2] == len(chunks[-1][1])
            chunks[-1][1].append(r)
    return chunks


def counts(chunks):
    """Per-kernel profiler counts (in the order of _lib.KERNELS) of a plan, by the profiler's rule: one event pair
    around the k_norm launch, the StateInit stage (however many launches), every update launch, every combine
    launch (after StateInit and every update but the last) and the one launch of a one-launch forward."""
    c = [0] * len(_lib.KERNELS)
    for head, stages in chunks:
        num_init, num_it, norm_pre = head[H_NUM_INIT], head[H_NUM_IT], head[H_NORM_PRE]
        one_launch, combine = head[14], head[15]
        assert len(stages) == num_init + num_it
        c[K_NORM] += norm_pre
        if one_launch:
            c[stages[0][4]] += 1
            continue
        c[stages[0][4]] += 1
        for s in stages[num_init:]:
            c[s[4]] += 1
        c[K_COMBINE] += combine * num_it
    return c


def check_records(chunks, batch, users, cus):
    assert sum(head[1] for head, _ in chunks) == batch
    assert [head[0] for head, _ in chunks] == [sum(h[1] for h, _ in chunks[:i]) for i in range(len(chunks))]
    for head, stages in chunks:
        one_launch, grid = head[14], head[H_GRID]
        if one_launch:
            # exactly one compute launch: the stages have no launch of their own and one kernel id
            assert grid == cus and all(s[11] == 0 and s[12] == 0 for s in stages)
            assert len({s[4] for s in stages}) == 1
        for s in stages:
            _, n, _, kind, _, tail, chp, one, pair, items, strips, grid, lds, order_rev, *_ = s
            assert items == n * users * strips
            if one_launch:
                continue
            assert order_rev == s[2] % 2 and lds > 0
            if kind in (RR, COL):       # persistent launches
                assert grid == min(items, cus) and not pair
                assert one == (kind == COL and items <= grid)
            else:
                assert not one and grid == (items // 2 if pair else items)
                assert not pair or items % 2 == 0


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("shape", SHAPES, ids=shape_key)
def test_plan_counts_equal_the_recorded_launches(lib, golden, shape):
    want = golden["cases"][shape_key(shape)]
    cs = combos(shape)
    assert len(want) == len(cs)
    for (num_it, fused, mask), w in zip(cs, want):
        chunks = plan(lib, shape, num_it, mask, fused)
        assert counts(chunks) == w, (num_it, fused, mask, chunks)
        check_records(chunks, shape[4], shape[2], 256)


@pytest.mark.parametrize("shape", BASELINE, ids=shape_key)
def test_baseline_shards_at_the_default_schedule(lib, golden, shape):
    chunks = plan(lib, shape, spec_of(shape).num_it, DEFAULT_MASK, 1)
    assert counts(chunks) == golden["baseline"][shape_key(shape)], chunks
    check_records(chunks, shape[4], shape[2], 256)


def test_f32x_plan_is_the_strip_tier(lib):
    chunks = plan(lib, ("nrx_rt", 4, 2, 4, 128), 2, DEFAULT_MASK, 1, precision=1)
    assert counts(chunks) == [0, 1, 2, 0, 0, 0, 0, 0, 0]
    check_records(chunks, 128, 2, 256)


def test_refusals(lib):
    fn = lib.nrx_debug_forward_plan
    plan(lib, SHAPES[0], 1, 0, 0)     # sets the signature
    desc = _lib.make_desc(spec_of(SHAPES[0]))
    sh = _lib.nrx_shape(4, 1, 48, 14)
    out = (ctypes.c_int32 * REC)()
    args = lambda **kw: [kw.get("desc", ctypes.byref(desc)), kw.get("shape", ctypes.byref(sh)), kw.get("precision", 0),
                         kw.get("num_it", 1), kw.get("mask", 0), kw.get("fused", 0), kw.get("cus", 256), 8,
                         kw.get("out", out), kw.get("cap", REC)]
    for bad in (dict(desc=None), dict(shape=None), dict(precision=2), dict(num_it=0), dict(num_it=3), dict(mask=128),
                dict(mask=-1), dict(fused=3), dict(cus=-1), dict(out=None)):
        assert fn(*args(**bad)) < 0, bad
    # cap too small: the length the plan takes comes back, nothing is written past cap
    need = 3 * REC     # the chunk's record, StateInit, one update
    guard = (ctypes.c_int32 * need)(*([77] * need))
    assert fn(*args(out=guard, cap=REC)) == need
    assert list(guard[REC:]) == [77] * (need - REC) and guard[2] == -1
    assert fn(*args(out=None, cap=0)) == need
