"""The memory side of the C ABI: poisoned workspaces, guard bands, sentinel outputs (needs an MI355X).

The value tests (test_gpu_topologies.py and the schedule tests) run every forward in the engine's
cached ``torch.empty`` workspace, the same shape several times over, into fresh outputs, with every
input alone in its own allocation.  A kernel that reads a workspace byte the current forward has
not written, writes a byte outside ``nrx_workspace_size`` / ``llr`` / ``h_ref``, leaves an output
element unwritten, or loads past the end of an input and multiplies by a zero weight, passes all of
them.  Here every forward runs again

  * in a workspace of exactly ``workspace_bytes(...)`` bytes that is the body of a guarded buffer
    (tests/memguard.py), prefilled with 0x00, 0xFF (NaN in every float type) and 0x7B (large and
    finite), with ``llr`` / ``h_ref`` guarded bodies prefilled with 0xFF -- outputs bit-identical
    to the plain run, finite everywhere, the 0xA5 guards untouched, head padding exactly 0, every
    tile equal to the first, the per-launch profile what ``dispatch_model`` says;
  * with every input as the body of a guarded buffer whose guards hold 0xFF / 0x7B -- outputs
    bit-identical to the plain run.

The other workspace users of the C ABI (K-best, 3-D LMMSE estimator, LLR statistics, channel
NMSE, the two covariance accumulators, the slot generator) get the first check at their smallest
existing test cases.  No run needs the fp64 oracle except the F = 132 gate of the separate norm
pass, a shape no other test covers.
"""
import dataclasses
import functools

import numpy as np
import pytest

from tests import test_gpu_topologies as T
from tests.helpers import make_aerial_case, run_oracle
from tests.memguard import FILLS, Guarded, guarded, guarded_input, guarded_out, same_bits
from tests.test_gpu_topologies import (COL, DEFAULT, SCHED_CASES, TOPOLOGIES, VARIO_A4, base_case, batch_past,
                                       dispatch_model, engine_for, expect, run_sched, tile, upload)

pytestmark = pytest.mark.gpu

VARIO = "a4_vario_u2"
LOOP_CASES = SCHED_CASES + [(VARIO, 12)]
MASKS = {"strip": 0, "rr": 3, "col": COL, "default": DEFAULT}


def _base(name, F):
    return base_case(name, F, VARIO_A4 if name == VARIO else None)


def _mask(label, F):
    return MASKS[label] | (64 if label == "col" and F > 48 else 0)


def expect_f32x(case):
    """profile of a parity-mode forward: the strip launch loop of Launch<P64>::run (nrx_launch.inc)"""
    U, F = case.active.shape[1], case.y.shape[1]
    n = dict.fromkeys(T._lib.KERNELS, 0)
    n_it = case.num_it or case.spec.num_it
    n["norm"] = 1 if F * 14 * 2 * case.spec.num_rx_ant // 4 > 8192 else 0
    n["state_init"], n["state_update"], n["combine"] = 1, n_it, n_it if U > 2 else 0
    return n


def check_outputs(case, llr, h, base_llr, base_h, label):
    spec = case.spec
    assert same_bits(llr, base_llr), (label, "llr differs from the plain run",
                                      float(np.nanmax(np.abs(llr - base_llr))), int(np.isnan(llr).sum()))
    assert np.isfinite(llr).all(), (label, "llr elements left unwritten")
    if base_h is not None:
        assert same_bits(h, base_h), (label, "h_ref differs from the plain run", int(np.isnan(h).sum()))
        assert np.isfinite(h).all(), (label, "h_ref elements left unwritten")
    if not spec.masking and len(set(spec.bits)) > 1:
        for m, nb in enumerate(spec.bits):
            assert np.all(llr[m, ..., nb:] == 0.0), (label, "head padding", m)
    if llr.shape[1] > 3 and llr.shape[1] % 3 == 0:
        for b in range(3, llr.shape[1], 3):
            assert same_bits(llr[:, b:b + 3], llr[:, :3]), (label, "tile", b)
            assert base_h is None or same_bits(h[b:b + 3], h[:3]), (label, "tile", b)


def contract(case, mask, fused=False, precision="f16", fills=FILLS, counts=None, want_h=True, mcs_mask="case",
             dev=None, label="", **kw):
    """The plain run, then one run per fill in an exactly sized guarded workspace with guarded 0xFF
    outputs; returns the plain run's (llr, h)."""
    import torch
    eng = engine_for(case)
    B, U, F = case.active.shape[0], case.active.shape[1], case.pe.shape[1]
    dev = dev if dev is not None else upload(case)
    common = dict(fused=fused, want_h=want_h, mcs_mask=mcs_mask, precision=precision, dev=dev, **kw)
    base_llr, base_h, prof = run_sched(case, mask, **common)
    if counts is not None:
        assert prof == counts, (label, prof, counts)
    check_outputs(case, base_llr, base_h, base_llr, base_h, f"{label} plain")
    nbytes = eng.workspace_bytes(B, U, F, precision, kw.get("y_layout", "cgnn"))
    for fill in fills:
        tag = f"{label} {precision} fill {fill:#04x}"
        ws = Guarded(nbytes, fill)
        llr_t, llr_g = guarded_out(base_llr.shape)
        h_t, h_g = guarded_out(base_h.shape) if want_h else (None, None)
        llr, h, prof_g = run_sched(case, mask, workspace=ws.body, out=(llr_t, h_t), **common)
        assert llr_t.data_ptr() == llr_g.body.data_ptr() and ws.body.numel() == nbytes
        assert prof_g == prof, (tag, prof_g, prof)
        ws.check(f"{tag}: workspace of {nbytes} bytes")
        llr_g.check(f"{tag}: llr")
        if want_h:
            h_g.check(f"{tag}: h_ref")
        check_outputs(case, llr, h, base_llr, base_h, tag)
    torch.cuda.synchronize()
    return base_llr, base_h


# ---------------------------------------------------------------- the helper itself
def test_guarded_buffer():
    import torch
    body, check = guarded(1000, 0x7B)
    assert body.numel() == 1000 and body.data_ptr() % 256 == 0 and bool((body == 0x7B).all())
    check()
    g = Guarded(1000, 0xFF)
    v = g.view(torch.float32, (250,))
    assert bool(torch.isnan(v).all()) and bool(torch.isnan(g.body.view(torch.float16)).all())
    assert bool(torch.isnan(g.body.view(torch.float64)).all())
    g.refill(0x7B)
    for dt in (torch.float16, torch.float32, torch.float64):
        assert bool(torch.isfinite(g.body.view(dt)).all()) and float(g.body.view(dt).abs().min()) > 6e4
    g.check()
    for off in (g.guard - 1, g.guard + 1000, g.guard + 1023, g.buf.numel() - 1):   # the alignment tail is guarded
        g.buf[off] = 0
        with pytest.raises(AssertionError):
            g.check()
        g.buf[off] = 0xA5
    g.check()


# ---------------------------------------------------------------- 2. launch-loop schedules
@pytest.mark.parametrize("sched", list(MASKS))
@pytest.mark.parametrize("name,F", LOOP_CASES)
def test_launch_loop(name, F, sched):
    base = _base(name, F)
    case = tile(base, batch_past(base, 1))
    mask = _mask(sched, F)
    tier, counts = expect(case, mask, False)
    assert tier == "strips24", tier
    n_it, one_head = base.num_it or base.spec.num_it, base.spec.num_llr_heads == 1
    if sched == "rr":
        assert counts["state_update_rr"] == (n_it if one_head else n_it - 1)
    if sched == "col":
        assert counts["state_update_col"] == (n_it if one_head else n_it - 1)
        assert counts["state_init_col"] == (1 if base.spec.num_rx_ant == 4 else 0)
    contract(case, mask, counts=counts, label=f"{name} F{F} {sched}")


# ---------------------------------------------------------------- 2. one-launch forwards
@pytest.mark.parametrize("name,F", [c for c in LOOP_CASES if c[0] != "a6_mask8_u16"])
def test_one_launch_forward(name, F):
    base = _base(name, F)
    case = tile(base, batch_past(base, 2))
    tier, counts = expect(case, DEFAULT, "force")
    assert tier == "k_forward" and counts["forward"] == 1, (tier, counts)
    contract(case, DEFAULT, fused="force", counts=counts, label=f"{name} F{F} k_forward")
    engine_for(case).check()


def test_one_launch_column_forward():
    name, F, mask = "a4_noh_u2", 48, DEFAULT | 32
    base = _base(name, F)
    spec, U = base.spec, base.active.shape[1]
    cus = T.cu_count()
    pick = [B for B in range(3, cus + 1, 3)
            if dispatch_model(spec, B, U, F, spec.num_it, mask, 1, cus)[0] == "fwd_col"]
    assert pick, f"no batch reaches k_fwd_col on {cus} CUs"
    B = pick[0]
    assert B * U * 3 > cus and B * U <= cus          # above the 16-row latency tier, at most one item per CU
    case = tile(base, B)
    tier, counts = expect(case, mask, True)
    assert tier == "fwd_col" and counts["forward_col"] == 1, (tier, counts)
    contract(case, mask, fused=True, counts=counts, label=f"{name} F{F} k_fwd_col B{B}")
    engine_for(case).check()


# ---------------------------------------------------------------- 2. latency tiers, parity mode
@pytest.mark.parametrize("precision", ["f16", "f32x"])
@pytest.mark.parametrize("name", list(TOPOLOGIES))
def test_small_grid(name, precision):
    case = _base(name, 20)
    if precision == "f16":
        tier, counts = expect(case, DEFAULT, True)
        assert tier == ("strips24" if case.spec.num_llr_heads == 3 else "strips8"), tier
    else:
        counts = expect_f32x(case)
    contract(case, DEFAULT, fused=True, precision=precision, counts=counts, label=f"{name} F20")


# ---------------------------------------------------------------- 2. separate norm pass
@functools.lru_cache(maxsize=None)
def _norm_case(F):
    base = _base("a9_b5_u7", F)
    y = base.y.copy()
    y[1] = 0.0                                        # the divide-no-nan branch of the slot norm
    return dataclasses.replace(base, y=y)


@pytest.mark.parametrize("precision", ["f16", "f32x"])
@pytest.mark.parametrize("F,norm", [(132, 1), (130, 0)])
def test_norm_pass(F, norm, precision):
    # F 14 2A / 4 = 8316 > 8192 at F = 132: k_norm writes norm[B]; 8190 at F = 130: the slot norm is
    # computed inside the StateInit kernels and the norm[B] region must be neither written nor read
    case = _norm_case(F)
    assert (F * 14 * 18 // 4 > 8192) == bool(norm)
    counts = expect(case, DEFAULT, True)[1] if precision == "f16" else expect_f32x(case)
    assert counts["norm"] == norm
    llr, h = contract(case, DEFAULT, fused=True, precision=precision, counts=counts, label=f"norm F{F}")
    if F == 132 and precision == "f32x":
        T.gate_f32x(run_oracle(case), T.split_heads(case.spec, llr, h))


# ---------------------------------------------------------------- 2. NULL h_ref and mcs_mask
@pytest.mark.parametrize("sched", ["strip", "default"])
def test_null_h_ref_and_mcs_mask(sched):
    base = _base("a3_noh_3heads_u5", 12)
    case = tile(base, batch_past(base, 1))
    counts = expect(case, MASKS[sched], False)[1]
    llr, h = contract(case, MASKS[sched], counts=counts, fills=(0xFF,), want_h=False, mcs_mask=None,
                      label=f"NULL h_ref / mcs_mask {sched}")
    assert h is None
    # mcs_mask = NULL is the one-hot mask on MCS 0
    m = np.zeros_like(case.mcs_mask)
    m[..., 0] = 1
    want, _, _ = run_sched(dataclasses.replace(case, mcs_mask=m), MASKS[sched], want_h=False)
    assert same_bits(llr, want)


# ---------------------------------------------------------------- 2. nrx_forward_ex layouts
@pytest.mark.parametrize("precision", ["f32x", "f16"])
@pytest.mark.parametrize("layout", ["sionna", "split"])
def test_y_layouts(layout, precision):
    import torch
    case = _base("a3_noh_3heads_u5", 20)
    eng, A = engine_for(case), case.spec.num_rx_ant
    counts = expect(case, DEFAULT, True)[1] if precision == "f16" else expect_f32x(case)
    want, want_h, _ = run_sched(case, DEFAULT, fused=True, precision=precision)
    dev = upload(case)
    re, im = np.ascontiguousarray(case.y[..., :A]), np.ascontiguousarray(case.y[..., A:])
    if layout == "sionna":
        grid = np.transpose(re + 1j * im, (0, 3, 2, 1))[:, None].astype(np.complex64)     # [B,1,A,14,F]
        dev["y"], kw = torch.from_numpy(np.ascontiguousarray(grid)).cuda(), dict(y_layout="sionna")
    else:
        dev["y"], kw = torch.from_numpy(re).cuda(), dict(y_layout="split", y_imag=torch.from_numpy(im).cuda())
    # the CGNN-layout copy of y sits in front of the forward's own workspace
    assert eng.workspace_bytes(3, 5, 20, precision, layout) > eng.workspace_bytes(3, 5, 20, precision)
    llr, h = contract(case, DEFAULT, fused=True, precision=precision, counts=counts, dev=dev,
                      label=f"y layout {layout}", **kw)
    assert same_bits(llr, want) and same_bits(h, want_h)


# ---------------------------------------------------------------- 2. Aerial forward
@functools.lru_cache(maxsize=None)
def _aerial(prbs):
    return make_aerial_case("nrx_rt", batch=2, users=2, prbs=prbs)


@pytest.mark.parametrize("precision", ["f16", "f32x"])
@pytest.mark.parametrize("prbs", [1, 4])
def test_aerial_forward(prbs, precision):
    import torch
    ac = _aerial(prbs)
    case, eng = ac.case, engine_for(ac.case)
    B, U, F = 2, 2, 12 * prbs
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in ac.inputs.items()}
    args = (t["y_real"], t["y_imag"], t["h_ls_real"], t["h_ls_imag"], t["dmrs_port_mask"], t["dmrs_ofdm_pos"],
            t["dmrs_subcarrier_pos"])
    counts = expect(case, DEFAULT, True)[1] if precision == "f16" else expect_f32x(case)

    def run(**kw):
        eng.profile(True)
        llr, h = eng.forward_aerial(*args, num_it=case.num_it, precision=precision, **kw)
        torch.cuda.synchronize()
        prof = {k: v[0] for k, v in eng.profile_read().items()}
        eng.profile(False)
        eng.check()
        assert prof == counts, (prof, counts)
        return llr.cpu().numpy(), h.cpu().numpy()

    base_llr, base_h = run()
    assert np.isfinite(base_llr).all() and np.isfinite(base_h).all()
    nbytes = eng.aerial_workspace_bytes(B, U, F, t["dmrs_ofdm_pos"].shape[1], t["dmrs_subcarrier_pos"].shape[1],
                                        precision)
    assert nbytes > eng.workspace_bytes(B, U, F, precision)
    for fill in FILLS:
        tag = f"aerial prbs {prbs} {precision} fill {fill:#04x}"
        ws = Guarded(nbytes, fill)
        llr_t, llr_g = guarded_out(base_llr.shape)
        h_t, h_g = guarded_out(base_h.shape)
        llr, h = run(workspace=ws.body, out=(llr_t, h_t))
        for g, what in ((ws, "workspace"), (llr_g, "llr"), (h_g, "h_hat")):
            g.check(f"{tag}: {what}")
        assert same_bits(llr, base_llr) and same_bits(h, base_h), tag
        assert np.isfinite(llr).all() and np.isfinite(h).all(), tag


# ---------------------------------------------------------------- 2. one workspace, two shapes
@pytest.mark.parametrize("order,fill", [((0, 1), 0xFF), ((1, 0), 0x7B)])
def test_reuse_across_shapes(order, fill):
    cases = []
    for name, F in (("a9_b5_u7", 60), ("a4_noh_u2", 12)):
        base = _base(name, F)
        case = tile(base, batch_past(base, 1))
        dev = upload(case)
        counts = expect(case, DEFAULT, False)[1]
        llr, h, prof = run_sched(case, DEFAULT, dev=dev)
        assert prof == counts
        B, U = case.active.shape
        cases.append((case, dev, counts, llr, h, engine_for(case).workspace_bytes(B, U, F)))
    ws = Guarded(max(c[5] for c in cases), fill)
    for i in order:                                    # back to back, the workspace not refilled between
        case, dev, counts, want, want_h, _ = cases[i]
        llr_t, llr_g = guarded_out(want.shape)
        h_t, h_g = guarded_out(want_h.shape)
        llr, h, prof = run_sched(case, DEFAULT, dev=dev, workspace=ws.body, out=(llr_t, h_t))
        assert prof == counts, (i, prof, counts)
        for g in (ws, llr_g, h_g):
            g.check(f"reuse {order} case {i}")
        check_outputs(case, llr, h, want, want_h, f"reuse {order} case {i}")


# ---------------------------------------------------------------- 2. graph replay
def test_graph_replay():
    import torch
    base = _base("a4_noh_u2", 12)
    case = tile(base, batch_past(base, 1))
    eng = engine_for(case)
    B, U = case.active.shape
    counts = expect(case, DEFAULT, False)[1]
    dev = upload(case)
    want, want_h, prof = run_sched(case, DEFAULT, dev=dev)
    assert prof == counts and counts["state_init_col"] == 1 and counts["state_update_col"] == 2
    ws = Guarded(eng.workspace_bytes(B, U, 12), 0x7B)
    llr_t, llr_g = guarded_out(want.shape)
    h_t, h_g = guarded_out(want_h.shape)
    fwd = lambda: eng.forward(dev["y"], dev["pe"], dev["h_hat"], dev["active"], dev["mcs_mask"], num_it=case.num_it,  # noqa: E731
                              precision="f16", workspace=ws.body, out=(llr_t, h_t))
    eng.fused_config(enable=False)
    eng.update_schedule(DEFAULT)
    try:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            fwd()                                      # warm-up
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                fwd()
            g.replay()
            first = (llr_t.cpu().numpy(), h_t.cpu().numpy())
            ws.refill(0xFF)                            # stream-ordered fills on the replay's stream
            llr_g.refill(0xFF)
            h_g.refill(0xFF)
            g.replay()
            second = (llr_t.cpu().numpy(), h_t.cpu().numpy())
            st.synchronize()
    finally:
        eng.fused_config(enable=True)
        eng.update_schedule(DEFAULT)
    for tag, (llr, h) in (("first replay", first), ("replay after the 0xFF refill", second)):
        check_outputs(case, llr, h, want, want_h, tag)
    for gb in (ws, llr_g, h_g):
        gb.check("graph replay")
    eng.check()


# ---------------------------------------------------------------- 3. inputs between NaN guards
def _guarded_inputs(case, guard_byte):
    dev, guards = {}, []
    for k, t in upload(case).items():
        if t is None:
            dev[k] = None
            continue
        dev[k], g = guarded_input(t, guard_byte)
        guards.append((k, g))
    return dev, guards


def _inputs_between_guards(case, mask, fused, precision, counts, label):
    want, want_h, prof = run_sched(case, mask, fused=fused, precision=precision)
    assert prof == counts, (label, prof, counts)
    for guard_byte in (0xFF, 0x7B):
        dev, guards = _guarded_inputs(case, guard_byte)
        llr, h, prof = run_sched(case, mask, fused=fused, precision=precision, dev=dev)
        tag = f"{label} {precision} input guards {guard_byte:#04x}"
        assert prof == counts, (tag, prof, counts)
        check_outputs(case, llr, h, want, want_h, tag)
        for k, g in guards:
            g.check(f"{tag}: {k}")                     # and no input was written


@pytest.mark.parametrize("precision", ["f16", "f32x"])
@pytest.mark.parametrize("name", ["a1_qpsk_u1", "a3_noh_3heads_u5", "a9_b5_u7"])
def test_inputs_between_guards_small(name, precision):
    case = _base(name, 20)
    counts = expect(case, DEFAULT, True)[1] if precision == "f16" else expect_f32x(case)
    _inputs_between_guards(case, DEFAULT, True, precision, counts, f"{name} F20")


@pytest.mark.parametrize("sched", ["strip", "default"])
def test_inputs_between_guards_launch_loop(sched):
    base = _base("a4_noh_u2", 12)
    case = tile(base, batch_past(base, 1))
    tier, counts = expect(case, MASKS[sched], False)
    assert tier == "strips24"
    _inputs_between_guards(case, MASKS[sched], False, "f16", counts, f"a4_noh_u2 F12 {sched}")


# ---------------------------------------------------------------- 4. the other workspace users
def _i64(t):
    return t.cpu().numpy().view(np.int64)


def _over_fills(run, nbytes, label):
    """``run(workspace or None) -> bytes of every output``: the plain call and one call per fill
    in an exactly sized guarded workspace give the same bytes, and the guards hold."""
    want = run(None)
    sizes = nbytes() if callable(nbytes) else nbytes
    sizes = sizes if isinstance(sizes, tuple) else (sizes,)
    assert all(n > 0 for n in sizes), (label, sizes)
    for fill in FILLS:
        gs = [Guarded(n, fill) for n in sizes]
        got = run(gs[0].body if len(gs) == 1 else tuple(g.body for g in gs))
        for g in gs:
            g.check(f"{label} fill {fill:#04x}: workspace of {g.nbytes} bytes")
        assert got == want, f"{label} fill {fill:#04x}: outputs differ from the plain call"


@pytest.mark.parametrize("name", ["K1", "K6"])
def test_kbest_workspace(name):
    import torch
    from neural_rx_amd.kbest import KBestDetector
    from tests import test_gpu_kbest as TK
    p, no = TK._params(name)
    sb, _ = TK._slots(name)
    det = KBestDetector()

    def run(ws):
        out, g = guarded_out((1,) + tuple(sb.h.shape[:4]) + (max(p.mcs_bits),))
        det(sb.y, sb.h, sb.active, sb.mcs, p.mcs_bits, no, p.dmrs_symbols, out=out, workspace=ws)
        torch.cuda.synchronize()
        g.check(f"kbest {name}: llr")
        assert bool(torch.isfinite(out).all())
        return out.cpu().numpy().tobytes()

    _over_fills(run, lambda: det.last_workspace_bytes, f"kbest {name}")


@pytest.mark.parametrize("name", ["K2", "K3"])
def test_chest_lmmse3_workspace(name):
    # K2: odd F, 7 / 6 pilots, partial tiles; K3: nd = 3, inactive users
    import torch
    from neural_rx_amd.chest import ChannelEstimator
    from tests import test_gpu_chest3 as T3
    sb, _ = T3._slots(name)
    est = ChannelEstimator("lmmse3", T3._params(name), tables=T3._design(name))

    def run(ws):
        out, g = guarded_out(tuple(sb.h_hat.shape))
        est(sb, T3._no(name), out=out, workspace=ws)
        torch.cuda.synchronize()
        g.check(f"lmmse3 {name}: h_out")
        assert bool(torch.isfinite(out).all())
        return out.cpu().numpy().tobytes()

    _over_fills(run, lambda: est.last_workspace_bytes, f"lmmse3 {name}")


@pytest.mark.parametrize("name,shift", [("S1", False), ("S1", True), ("S2", False), ("S4", False)])
def test_llr_stats_workspace(name, shift):
    # S1 shifted: the scalar rows; S2: odd F, three MCS, an inactive user; S4: F = 2 strips + 5
    import torch
    from neural_rx_amd import softmetrics as SM
    from tests import test_gpu_softmetrics as TS
    H, B, U, F, bs, mcs_bits, dmrs, _, scales = TS.CASES[name]
    (llr, bits, active, mcs), _ = TS._inputs(name)
    size = []

    def dev(a):
        t = torch.from_numpy(np.array(a)).cuda()
        if not shift:
            return t
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        buf[1:] = t.reshape(-1)
        return buf[1:].view(t.shape)

    d = [dev(a) for a in (llr, bits, active, mcs)]

    def run(ws):
        acc = SM.SoftAccumulator(U, mcs_bits, scales)
        acc.add_llr(*d, dmrs, workspace=ws)
        torch.cuda.synchronize()
        size.append(acc.last_workspace_bytes)
        return _i64(acc.i64).tobytes() + _i64(acc.f64).tobytes()

    _over_fills(run, lambda: size[0], f"llr_stats {name}")


@pytest.mark.parametrize("name,shift", [("N1", False), ("N2", True), ("N3", False)])
def test_chest_nmse_workspace(name, shift):
    import torch
    from neural_rx_amd import softmetrics as SM
    from tests import test_gpu_softmetrics as TS
    B, U, F, A, mask, _ = TS.NMSE_CASES[name]
    he, h, active, _ = TS._channels(name)
    size = []

    def dev(a, off):
        if not off:
            return torch.from_numpy(a).cuda()
        buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(a).reshape(-1).cuda()
        return buf[1:].view(a.shape)

    d = (dev(he, shift), dev(h, shift), dev(active, False))

    def run(ws):
        acc = SM.SoftAccumulator(U, (4,))
        acc.add_channel(*d, mask, workspace=ws)
        torch.cuda.synchronize()
        size.append(acc.last_workspace_bytes)
        return _i64(acc.i64).tobytes() + _i64(acc.f64).tobytes()

    _over_fills(run, lambda: size[0], f"chest_nmse {name}")


@pytest.mark.parametrize("name", ["K1", "K2"])
def test_covariance_workspaces(name):
    # nrx_cov_accumulate and nrx_cov_space_accumulate, each in its own guarded workspace; K2: odd F
    import torch
    from neural_rx_amd.chest import CovarianceEstimator
    from tests import test_gpu_chest as TC
    sb, _ = TC._slots(name)
    size = []

    def run(ws):
        cov = CovarianceEstimator(TC._params(name))
        cov.accumulate(sb, workspace=ws)
        torch.cuda.synchronize()
        size.append(cov.last_workspace_bytes)
        return _i64(cov.acc).tobytes() + _i64(cov.acc_s).tobytes()

    _over_fills(run, lambda: size[0], f"covariance {name}")


def _gen_bytes(sb):
    return b"".join(v.cpu().numpy().tobytes() for _, v in sorted(vars(sb).items()) if v is not None)


@pytest.mark.parametrize("which", ["plain", "odd_width", "aerial", "chan"])
def test_generator_workspace(which):
    # nrx_generate_slots (plain; F = 13 with one tap and slot offset 2^33; the Aerial outputs) and
    # nrx_generate_slots_ex (two profiles, correlated antennas)
    import torch
    from neural_rx_amd.generator import GenParams, SlotGenerator, rx_correlation
    aerial, off, B, no = False, 5, 3, 0.05
    if which == "plain":
        p = GenParams.from_config("nrx_rt", num_tx=1, num_prbs=1, num_rx_ant=4, seed=11)
    elif which == "odd_width":
        p = GenParams(num_tx=2, num_subcarriers=13, num_rx_ant=2, dmrs_symbols=(2,), cdm_group=(1, 0), mcs_bits=(2,),
                      num_taps=1, num_sinusoids=1, max_delay_s=0.0, max_doppler_hz=0.0, seed=2**40 + 3)
        off, B, no = 2**33, 2, 0.0
    elif which == "aerial":
        p, aerial, B = GenParams.from_config("nrx_rt", seed=9), True, 2
    else:
        p = GenParams(num_tx=2, num_subcarriers=24, num_rx_ant=4, seed=11,
                      user_profiles=[(420e-9, 400.0), (1270e-9, 100.0)], rx_corr=rx_correlation(4, 0.9))
    gen = SlotGenerator(p, want_h=True, aerial=aerial)
    assert p.correlated == (which == "chan")
    out = gen(B, no, slot_offset=off)                  # the output tensors, written anew by every run

    def run(ws):
        for v in vars(out).values():
            if v is not None:
                v.view(torch.uint8).fill_(0xFF)
        sb = gen(B, no, slot_offset=off, out=out, workspace=ws)
        torch.cuda.synchronize()
        return _gen_bytes(sb)

    _over_fills(run, gen.workspace_bytes(B), f"generator {which}")
