"""The CGNN engine over the topology range nrx_create accepts (needs an MI355X).

check_desc (nrx_model.cpp) / check_shape (nrx_api.cpp) accept 1..16 rx antennas, 1..8 bits per head, up to 8 MCS
with masking (3 heads without), models with and without h_hat and 1..16 users; the rest of the
GPU suite runs 4 and 16 antennas, 4 / 6 bits, h_hat always, one-hot MCS masks and U in {1, 2, 3,
4, 8}.  The six seeded topologies below reach what that leaves out:

  a1_qpsk_u1        2A = 2: float2 loads of init_user, 6 pad channels of the 8-wide antenna
                    block, 2-wide scalar LLR / ChEst stores
  a3_noh_3heads_u5  2A = 6 (float2 loads, nvalid & 3 store tail), no h_hat, three heads of 1 / 3 /
                    8 bits, a soft MCS mask with exact one-hot rows among it (the wm == 0 skip and
                    the weighted sum in one launch), odd U through the combine pass; three heads
                    do not fit the 8- / 16-row strip images, so every size runs the 24-row tier
  a4_noh_u2         use_h = 0 in the column StateInit (2A = 8) and in the one-launch forward
  a6_mask8_u16      2A = 12 in a 16-wide block, 8 MCS on one masked head, U = kMaxUsers (past the
                    one-launch forward's 8 users: the dispatcher must fall back)
  a8_64qam_u3       2A = 16 = A2P = CHP, 2 of 3 trained iterations
  a9_b5_u7          2A = 18 in a 32-wide block (14 pad channels, CHP = 32, odd A), 5 bits, U = 7

Every case is three distinct slots (seeded activity: one slot with a single active user, at least
one inactive (slot, user), no empty slot unless U = 1), tiled where a larger batch is needed, so
the fp64 oracle only ever runs on three slots.  Which kernel must run each stage is derived by
``dispatch_model`` below -- a restatement of the applicability functions of nrx_dispatch.hip,
nrx_launch.inc, nrx_k_col.hip and nrx_k_rr.hip -- and asserted from the per-launch profile, so no
case passes by quietly taking another kernel.

Gates.  f32x: the project's (LLR max-abs < 1e-3, h max-abs < 1e-4, tests/test_gpu_parity.py).
f16: the project's (10 % of max|LLR|, 2 % RMS, flips) plus a tight one: with seeded weights the
f16 roundings themselves move the LLRs far less than the project gate allows, so the engine's
deviation E from the fp64 oracle is held to K_TIGHT times the deviation R of the oracle run under
the f16 rounding model of tests/f16_ref.py (stored activations and kernels in f16, depthwise sum
in f16 in the kernels' order, matmuls in f64): E_rel <= K_TIGHT * R_rel and E_rms <= K_TIGHT *
R_rms, K_TIGHT * R never above the project gate.  K_TIGHT is twice the largest ratio measured
below, rounded up (seed-to-seed spread, the f32 MFMA accumulation the model does not reproduce).

Measured on an MI355X (256 CUs), llr_rel / llr_rms_rel in % of max|LLR| / RMS LLR against the
fp64 oracle; "small" = the three slots at F = 20 (test_f16_small_grid), "F12" / "F60" = the
tiled batch (test_f16_schedules), "mcs0" = one-hot on MCS 0 (the mcs_mask = None tests):

  case                            E_rel  E_rms  R_rel  R_rms  E/R rel  E/R rms
  a1_qpsk_u1 small                0.206  0.153  0.172  0.151     1.20     1.01
  a3_noh_3heads_u5 small          0.148  0.141  0.144  0.138     1.03     1.02
  a4_noh_u2 small                 0.120  0.101  0.108  0.098     1.11     1.03
  a6_mask8_u16 small              0.162  0.142  0.192  0.139     0.84     1.02
  a8_64qam_u3 small               0.244  0.132  0.163  0.129     1.50     1.02
  a9_b5_u7 small                  0.150  0.149  0.163  0.147     0.92     1.02
  a1_qpsk_u1 F12                  0.167  0.160  0.164  0.151     1.02     1.06
  a3_noh_3heads_u5 F12            0.132  0.142  0.124  0.135     1.07     1.05
  a4_noh_u2 F12                   0.151  0.104  0.134  0.100     1.12     1.04
  a6_mask8_u16 F12                0.161  0.139  0.154  0.137     1.05     1.02
  a8_64qam_u3 F12                 0.150  0.130  0.146  0.128     1.02     1.01
  a9_b5_u7 F12                    0.161  0.144  0.144  0.140     1.11     1.03
  a4_noh_u2 F60                   0.118  0.102  0.112  0.099     1.06     1.03
  a9_b5_u7 F60                    0.155  0.150  0.145  0.147     1.06     1.03
  a3_noh_3heads_u5 mcs0 small     0.158  0.148  0.128  0.142     1.23     1.04
  a4_vario_u2 mcs0 F12            0.141  0.155  0.124  0.146     1.13     1.06

The largest ratio is 1.50 (the max-abs figure of a8_64qam_u3, one element; its RMS ratio and its
F = 12 ratios sit with the others), so K_TIGHT = 3; 3 R stays below 0.6 % of max|LLR| and 0.5 % RMS.

The one-launch forward (k_forward) applies from two items per CU, so its runs tile the three slots
to the smallest multiple of 3 with B U ceil(F / 24) >= 2 CUs; the other schedules run at the
smallest multiple of 3 past one item per CU.
"""
import dataclasses
import math

import numpy as np
import pytest

from neural_rx_amd import _lib
from neural_rx_amd import weights as W
from neural_rx_amd.config import get_config, spec_from_config
from oracle import pe_ref
from tests.f16_ref import f16_rounded_oracle
from tests.helpers import Case, compare, run_engine, run_oracle
from tests.test_gpu_parity import (F16_FLIP_CONF_TOL, F16_FLIP_TOL, F16_REL_TOL, F16_RMS_TOL, F32X_H_TOL,
                                   F32X_LLR_TOL)

pytestmark = pytest.mark.gpu

K_TIGHT = 3

COL = 4 | 8 | 16
DEFAULT = 29

TOPOLOGIES = {
    "a1_qpsk_u1": dict(spec=dict(num_rx_ant=1, use_h_hat=True, bits=(2,), masking=False, num_it=2), users=1),
    "a3_noh_3heads_u5": dict(spec=dict(num_rx_ant=3, use_h_hat=False, bits=(1, 3, 8), masking=False, num_it=2),
                             users=5, mask="soft"),
    "a4_noh_u2": dict(spec=dict(num_rx_ant=4, use_h_hat=False, bits=(4,), masking=False, num_it=2), users=2),
    "a6_mask8_u16": dict(spec=dict(num_rx_ant=6, use_h_hat=True, bits=(1, 2, 3, 4, 5, 6, 7, 8), masking=True,
                                   num_it=2), users=16),
    "a8_64qam_u3": dict(spec=dict(num_rx_ant=8, use_h_hat=True, bits=(6,), masking=False, num_it=3), users=3,
                        run_it=2),
    "a9_b5_u7": dict(spec=dict(num_rx_ant=9, use_h_hat=True, bits=(5,), masking=False, num_it=2), users=7),
}
# beside the six: Var-IO over 2A = 8, where the column StateInit runs one launch per MCS
VARIO_A4 = dict(spec=dict(num_rx_ant=4, use_h_hat=True, bits=(2, 4), masking=False, num_it=2), users=2)
SEEDS = {name: 3 + i for i, name in enumerate(TOPOLOGIES)}
WIDE = ("a4_noh_u2", "a9_b5_u7")          # also run at F = 60: two columns and a halo
SCHED_CASES = [(n, 12) for n in TOPOLOGIES] + [(n, 60) for n in WIDE]


# ---------------------------------------------------------------- cases
def random_activity(rng, slots, users):
    """[slots, users]: slot 0 has exactly one active user, slot 1 at least one inactive and one
    active user, no slot is empty (U = 1: the middle slot is, being the only way to be inactive)."""
    if users == 1:
        return np.array([[1.0], [0.0], [1.0]], np.float32)[:slots]
    act = (rng.random((slots, users)) < 0.6).astype(np.float32)
    act[0] = 0
    act[0, rng.integers(users)] = 1
    for b in range(1, slots):
        if act[b].sum() == 0:
            act[b, rng.integers(users)] = 1
    if act[1].sum() == users:
        act[1, rng.integers(users)] = 0
    return act


def topo_case(spec_overrides, users, F, batch, seed, active=None, mcs_mask=None, name="topo", num_it=None):
    spec = dataclasses.replace(spec_from_config(get_config("nrx_rt")), **spec_overrides)
    weights = W.seeded(spec, seed)
    rng = np.random.default_rng(seed + 1000 * F)
    a2 = 2 * spec.num_rx_ant
    y = rng.standard_normal((batch, F, 14, a2)).astype(np.float32)
    h_hat = rng.standard_normal((batch, users, F, 14, a2)).astype(np.float32) if spec.use_h_hat else None
    pe = pe_ref.pe_for_groups(F, 14, (2, 11), tuple(u % 2 for u in range(users)))
    if active is None:
        active = random_activity(rng, batch, users)
    if isinstance(mcs_mask, str) and mcs_mask == "soft":
        # Dirichlet rows; about a third forced to an exact one-hot (the first row always)
        mcs_mask = rng.dirichlet(np.ones(spec.num_mcs), size=(batch, users)).astype(np.float32)
        hot = rng.random((batch, users)) < 1.0 / 3.0
        hot[0, 0], hot[0, -1] = True, False
        mcs_mask[hot] = np.eye(spec.num_mcs, dtype=np.float32)[rng.integers(0, spec.num_mcs, size=int(hot.sum()))]
    elif mcs_mask is None:
        mcs_mask = np.eye(spec.num_mcs, dtype=np.float32)[rng.integers(0, spec.num_mcs, size=(batch, users))]
    return Case(name, None, spec, weights, y, pe, h_hat, np.asarray(active, np.float32),
                np.asarray(mcs_mask, np.float32), None, num_it)


def tile(case, batch):
    """The three slots repeated to ``batch`` slots (a multiple of 3)."""
    assert batch % 3 == 0 and case.y.shape[0] == 3
    r = lambda a: None if a is None else np.concatenate([a] * (batch // 3), axis=0)   # noqa: E731
    return dataclasses.replace(case, y=r(case.y), h_hat=r(case.h_hat), active=r(case.active),
                               mcs_mask=r(case.mcs_mask))


_ENGINES, _BASE, _REF = {}, {}, {}


def engine_for(case):
    """One engine per (spec, weight fingerprint)."""
    from neural_rx_amd.receiver import CGNNEngine
    key = (case.spec, tuple((np.shape(w), float(np.asarray(w, np.float64).ravel()[:16].sum())) for w in case.weights))
    if key not in _ENGINES:
        _ENGINES[key] = CGNNEngine(case.spec, case.weights)
    return _ENGINES[key]


def base_case(name, F, topo=None):
    """The three slots of a topology at grid width F (built once)."""
    if (name, F) not in _BASE:
        t = topo or TOPOLOGIES[name]
        _BASE[name, F] = topo_case(t["spec"], t["users"], F, 3, SEEDS.get(name, 11), mcs_mask=t.get("mask"),
                                   name=name, num_it=t.get("run_it"))
    return _BASE[name, F]


def references(case, key):
    """(fp64 oracle, its deviation under the f16 rounding model) of a three-slot case, computed once."""
    if key not in _REF:
        ref = run_oracle(case)
        _REF[key] = (ref, compare(ref, f16_rounded_oracle(case)))
    return _REF[key]


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------- which kernel runs what
def _align256(x):
    return (x + 255) & ~255


def dispatch_model(spec, B, U, F, num_it, mask, fused, cus):
    """(tier, {profile kernel: launches}) of one f16 forward: plan_forward (nrx_dispatch.hip)
    restated; ``fused`` = 0 off, 1 default, 2 forced."""
    a2, H, ninit, bmax = 2 * spec.num_rx_ant, spec.num_llr_heads, spec.num_init, spec.bits_max
    n = dict.fromkeys(_lib.KERNELS, 0)
    n["norm"] = 1 if F * 14 * a2 // 4 > 8192 else 0                        # kNormFusedMaxQ
    n["combine"] = num_it if U > 2 else 0                                  # kInlineUsers
    head_img = 24 * 1024 + 1024                                            # kHeadSlot + 1024
    for fo in (8, 16):                                                     # P16S, P16M
        if B * U * math.ceil(F / fo) <= cus and (H + 1) * head_img <= (fo + 6) * 4096:
            n["state_init"], n["state_update"] = 1, num_it
            return f"strips{fo}", n
    state = _align256(B * U * F * 14 * 56 * 2)
    gz = _align256(B * 8) + 4 * state + _align256(U * F * 14 * 56 * 2) < 1 << 30   # ws_bytes < kGzOob, pe16
    chp = 16 if a2 <= 16 else 32
    # rr_heads_fit: kHW2 + 256 (bits_max + chp) <= kRrExRows kRrExRow
    heads_rr = lambda c: bmax <= 16 and a2 <= c <= 32 and 33984 + 256 * (bmax + c) <= 14 * 3584   # noqa: E731
    col_init_ok = a2 == 8                                                  # init_cinp == 32 with it
    cstrips = 1 if F <= 48 else math.ceil(F / 44)                          # col_strips
    if fused and mask & 32 and U <= 2 and ninit == 1 and col_init_ok and gz and H == 1 and heads_rr(16) and \
            B * U * cstrips <= cus and 1 + num_it <= 9:
        n["forward_col"] = 1
        return "fwd_col", n
    if fused:
        items = B * U * math.ceil(F / 24)
        nls = ninit + num_it * (2 if U > 2 else 1)
        # heads: H <= 3 heads + ChEst fit the 30-slot strip image ((H + 1) 25 KB <= 120 KB)
        ok = items >= 2 * cus and U <= 8 and ninit + num_it <= 12 and nls <= 20 and a2 <= 32 and bmax <= 16 and \
            (H + 1) * head_img <= 30 * 4096
        if fused == 1:
            # the default takes only U <= 2 forwards of four stages or more (and then depends on
            # the readout layout, which this restatement leaves out)
            assert ninit + num_it < 4 or U > 2, "dispatch_model: default one-launch rule not restated"
            ok = False
        if ok:
            n["combine"] = 0                                               # combine stages run inside
            n["forward"] = 1
            return "k_forward", n
    n["state_init_col" if mask & 16 and col_init_ok else "state_init"] = 1
    for i in range(num_it):
        last = i == num_it - 1
        fits = not last or (H == 1 and heads_rr(chp))
        col = bool(mask & (8 if last else 4)) and gz and (cstrips == 1 or bool(mask & 64)) and fits
        rr = not col and bool(mask & (2 if last else 1)) and gz and fits
        n["state_update_col" if col else "state_update_rr" if rr else "state_update"] += 1
    return "strips24", n


def upload(case):
    """The case's input tensors on the device, keyed as run_sched's ``dev`` takes them."""
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    return {k: t(getattr(case, k)) for k in ("y", "pe", "h_hat", "active", "mcs_mask")}


def run_sched(case, mask, fused=False, want_h=True, mcs_mask="case", precision="f16", dev=None, **forward_kw):
    """One forward (f16 unless ``precision`` says otherwise) under a schedule mask; returns
    (llr_raw, h or None, profile counts).  ``dev``: the inputs already on the device (``upload``,
    or tensors placed by the caller), uploaded here otherwise; ``forward_kw`` goes on to
    ``CGNNEngine.forward`` (workspace=, out=, y_layout=, y_imag=)."""
    import torch
    eng = engine_for(case)
    d = dev if dev is not None else upload(case)
    eng.fused_config(enable=fused)
    eng.update_schedule(mask)
    try:
        eng.profile(True)
        llr, h = eng.forward(d["y"], d["pe"], d["h_hat"], d["active"],
                             d["mcs_mask"] if isinstance(mcs_mask, str) else mcs_mask,
                             num_it=case.num_it, precision=precision, want_h=want_h, **forward_kw)
        torch.cuda.synchronize()
        prof = {k: v[0] for k, v in eng.profile_read().items()}
        eng.profile(False)
        eng.check()                     # no dependency-wait timeout of a one-launch forward
    finally:
        eng.fused_config(enable=True)
        eng.update_schedule(DEFAULT)
    return llr.cpu().numpy(), None if h is None else h.cpu().numpy(), prof


def expect(case, mask, fused):
    B, U, F = case.y.shape[0], case.active.shape[1], case.y.shape[1]
    return dispatch_model(case.spec, B, U, F, case.num_it or case.spec.num_it, mask,
                          2 if fused == "force" else int(fused), cu_count())


def split_heads(spec, llr_raw, h):
    return {"llr": [llr_raw[0 if spec.masking else m, ..., :nb] for m, nb in enumerate(spec.bits)],
            "llr_raw": llr_raw, "h_hat": h}


def batch_past(case, items_per_cu):
    """Smallest multiple of 3 slots with B U ceil(F / 24) > CUs (1) / >= 2 CUs (2)."""
    U, F = case.active.shape[1], case.y.shape[1]
    per_slot = U * math.ceil(F / 24)
    need = cu_count() + 1 if items_per_cu == 1 else 2 * cu_count()
    return 3 * math.ceil(math.ceil(need / per_slot) / 3)


# ---------------------------------------------------------------- gates
def gate_f32x(ref, got):
    c = compare(ref, got)
    assert np.isfinite(got["llr_raw"]).all() and np.isfinite(got["h_hat"]).all()
    assert c["llr_maxabs"] < F32X_LLR_TOL, c
    assert c["h_maxabs"] < F32X_H_TOL, c
    return c


def gate_f16(ref, rdev, got, label):
    """The project's f16 gates and the tight gate against the f16-rounded oracle's deviation."""
    c = compare(ref, got)
    print(f"F16DEV {label:34s} E_rel {100 * c['llr_rel']:.4f} E_rms {100 * c['llr_rms_rel']:.4f} "
          f"R_rel {100 * rdev['llr_rel']:.4f} R_rms {100 * rdev['llr_rms_rel']:.4f} "
          f"ratio {c['llr_rel'] / rdev['llr_rel']:.2f} {c['llr_rms_rel'] / rdev['llr_rms_rel']:.2f} "
          f"flips {c['flip_rate']:.1e} {c['flip_rate_confident']:.1e} h {c['h_maxabs']:.2e}")
    assert np.isfinite(got["llr_raw"]).all() and np.isfinite(got["h_hat"]).all()
    assert c["llr_rel"] <= F16_REL_TOL, c
    assert c["llr_rms_rel"] <= F16_RMS_TOL, c
    assert c["flip_rate"] <= F16_FLIP_TOL, c
    assert c["flip_rate_confident"] <= F16_FLIP_CONF_TOL, c
    if K_TIGHT is not None:
        assert K_TIGHT * rdev["llr_rel"] <= F16_REL_TOL and K_TIGHT * rdev["llr_rms_rel"] <= F16_RMS_TOL, rdev
        assert c["llr_rel"] <= K_TIGHT * rdev["llr_rel"], (c, rdev)
        assert c["llr_rms_rel"] <= K_TIGHT * rdev["llr_rms_rel"], (c, rdev)
    return c


# ---------------------------------------------------------------- checks
@pytest.mark.parametrize("name", list(TOPOLOGIES))
def test_weight_layout_and_workspace(name):
    import ctypes
    case = base_case(name, 20)
    lib = _lib.load()
    d = _lib.make_desc(case.spec)
    n = ctypes.c_int32()
    assert lib.nrx_weight_layout(ctypes.byref(d), ctypes.byref(n), None, 0) == 0
    sizes = (ctypes.c_int64 * n.value)()
    assert lib.nrx_weight_layout(ctypes.byref(d), ctypes.byref(n), sizes, n.value) == 0
    assert list(sizes) == [w.size for w in W.seeded(case.spec)]
    eng = engine_for(case)
    U = case.active.shape[1]
    for prec in ("f16", "f32x"):
        assert eng.workspace_bytes(3, U, 20, prec) > 0
        assert eng.workspace_bytes(batch_past(base_case(name, 12), 2), U, 12, prec) > 0


def test_activity_and_mask_fixtures():
    # what the cases claim to hold: a slot with one active user, an inactive (slot, user), no empty
    # slot unless U = 1; the soft mask mixes exact one-hot rows with mixing rows
    for name, t in TOPOLOGIES.items():
        for F in (20, 12):
            act = base_case(name, F).active
            assert (act.sum(axis=1) == 1).any() and (act == 0).any(), name
            assert t["users"] == 1 or (act.sum(axis=1) >= 1).all(), name
    m = base_case("a3_noh_3heads_u5", 20).mcs_mask
    hot = (m == 1).any(axis=-1)
    assert hot.any() and not hot.all() and ((m > 0).sum(axis=-1)[~hot] == 3).all()
    np.testing.assert_allclose(m.sum(axis=-1), 1.0, atol=1e-6)


@pytest.mark.parametrize("name", list(TOPOLOGIES))
def test_f32x_parity(name):
    # B = 3, F = 20: no strip width divides 20 (the last strip is partial)
    case = base_case(name, 20)
    ref, _ = references(case, (name, 20))
    gate_f32x(ref, run_engine(case, "f32x", engine_for(case)))


@pytest.mark.parametrize("name", list(TOPOLOGIES))
def test_f16_small_grid(name):
    # the same three slots in f16: at most one item per CU, so the 8-row strip tier runs wherever
    # the heads fit its image (three heads do not: the 24-row tier under the default schedule)
    case = base_case(name, 20)
    ref, rdev = references(case, (name, 20))
    U = case.active.shape[1]
    assert 3 * U * math.ceil(20 / 8) <= cu_count()
    tier, counts = expect(case, DEFAULT, True)
    assert tier == ("strips24" if case.spec.num_llr_heads == 3 else "strips8"), tier
    llr, h, prof = run_sched(case, DEFAULT, fused=True)
    assert prof == counts, (tier, prof, counts)
    gate_f16(ref, rdev, split_heads(case.spec, llr, h), f"{name} small")


@pytest.mark.parametrize("name,F", SCHED_CASES)
def test_f16_schedules(name, F):
    base = base_case(name, F)
    ref, rdev = references(base, (name, F))
    spec, U = base.spec, base.active.shape[1]
    case = tile(base, batch_past(base, 1))
    wide = 64 if F > 48 else 0
    runs = {}
    for label, mask in (("strip", 0), ("rr", 3), ("col", COL | wide), ("default", DEFAULT)):
        tier, counts = expect(case, mask, False)
        assert tier == "strips24", (label, tier)
        llr, h, prof = run_sched(case, mask)
        assert prof == counts, (label, prof, counts)
        runs[label] = (llr, h)
    # the masks reach the kernels they are meant to: every update stage on the RR / column launch
    # where one head is read out (three heads keep the strip readout), the column StateInit at 2A = 8
    n_it = base.num_it or spec.num_it
    one_head = spec.num_llr_heads == 1
    assert expect(case, 3, False)[1]["state_update_rr"] == (n_it if one_head else n_it - 1)
    assert expect(case, COL | wide, False)[1]["state_update_col"] == (n_it if one_head else n_it - 1)
    assert expect(case, COL | wide, False)[1]["state_init_col"] == (1 if spec.num_rx_ant == 4 else 0)
    # the one-launch forward, from two items per CU; U = 16 is past its user limit
    fcase = tile(base, batch_past(base, 2))
    tier, counts = expect(fcase, DEFAULT, "force")
    assert tier == ("k_forward" if U <= 8 else "strips24"), tier
    llr, h, prof = run_sched(fcase, DEFAULT, fused="force")
    assert prof == counts, ("force", prof, counts)
    runs["force"] = (llr, h)
    llr0, h0 = runs["strip"]
    for label, (llr, h) in runs.items():
        # every tile equals the first, and the first equals the strip kernels' bit for bit
        assert np.array_equal(llr[:, :3], llr0[:, :3]), (label, np.abs(llr[:, :3] - llr0[:, :3]).max())
        assert np.array_equal(h[:3], h0[:3]), label
        for b in range(3, llr.shape[1], 3):
            assert np.array_equal(llr[:, b:b + 3], llr[:, :3]), (label, b)
            assert np.array_equal(h[b:b + 3], h[:3]), (label, b)
    gate_f16(ref, rdev, split_heads(spec, llr0[:, :3], h0[:3]), f"{name} F{F}")


@pytest.mark.parametrize("name", ["a3_noh_3heads_u5", "a4_noh_u2", "a9_b5_u7"])
def test_h_ref_null(name):
    # io.h_ref = NULL (want_h=False): the same LLRs, no ChEst output
    import torch
    small = base_case(name, 20)
    eng = engine_for(small)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    want = run_engine(small, "f32x", eng)["llr_raw"]
    llr, h = eng.forward(t(small.y), t(small.pe), t(small.h_hat), t(small.active), t(small.mcs_mask),
                         num_it=small.num_it, precision="f32x", want_h=False)
    assert h is None and np.array_equal(llr.cpu().numpy(), want)
    base = base_case(name, 12)
    for case, mask, fused in ((tile(base, batch_past(base, 1)), 0, False),
                              (tile(base, batch_past(base, 1)), DEFAULT, False),
                              (tile(base, batch_past(base, 2)), DEFAULT, "force")):
        tier, counts = expect(case, mask, fused)
        assert tier == ("k_forward" if fused else "strips24")
        want, _, _ = run_sched(case, mask, fused)
        llr, h, prof = run_sched(case, mask, fused, want_h=False)
        assert prof == counts, (prof, counts)
        assert h is None and np.array_equal(llr, want), (mask, fused)


def _one_hot0(case):
    m = np.zeros_like(case.mcs_mask)
    m[..., 0] = 1
    return dataclasses.replace(case, mcs_mask=m)


def test_mcs_mask_none_three_heads():
    # mcs_mask = NULL on a Var-IO model = one-hot on MCS 0
    import torch
    name = "a3_noh_3heads_u5"
    small = _one_hot0(base_case(name, 20))
    ref, rdev = references(small, (name, 20, "mcs0"))
    eng = engine_for(small)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    got = run_engine(small, "f32x", eng)
    gate_f32x(ref, got)
    llr, h = eng.forward(t(small.y), t(small.pe), None, t(small.active), None, num_it=None, precision="f32x")
    assert np.array_equal(llr.cpu().numpy(), got["llr_raw"]) and np.array_equal(h.cpu().numpy(), got["h_hat"])
    llr16, h16, _ = run_sched(small, DEFAULT, fused=True)
    gate_f16(ref, rdev, split_heads(small.spec, llr16, h16), f"{name} mcs0 small")
    llr, h, _ = run_sched(small, DEFAULT, fused=True, mcs_mask=None)
    assert np.array_equal(llr, llr16) and np.array_equal(h, h16)
    # past one item per CU: the strip kernels, the default schedule, the one-launch forward
    base = _one_hot0(base_case(name, 12))
    for case, mask, fused in ((tile(base, batch_past(base, 1)), 0, False),
                              (tile(base, batch_past(base, 1)), DEFAULT, False),
                              (tile(base, batch_past(base, 2)), DEFAULT, "force")):
        want, hw, _ = run_sched(case, mask, fused)
        llr, h, prof = run_sched(case, mask, fused, mcs_mask=None)
        assert prof == expect(case, mask, fused)[1]
        assert np.array_equal(llr, want) and np.array_equal(h, hw), (mask, fused)


def test_mcs_mask_none_column_state_init():
    # Var-IO over 2A = 8: the column StateInit runs one launch per MCS and must weigh them (1, 0)
    # without a mask, as the strip kernels do
    name = "a4_vario_u2"
    base = _one_hot0(base_case(name, 12, VARIO_A4))
    ref, rdev = references(base, (name, 12, "mcs0"))
    case = tile(base, batch_past(base, 1))
    assert expect(case, DEFAULT, False)[1]["state_init_col"] == 1
    want, hw, _ = run_sched(case, 0)
    for mask in (0, DEFAULT):
        llr, h, prof = run_sched(case, mask, mcs_mask=None)
        assert prof == expect(case, mask, False)[1]
        assert np.array_equal(llr, want) and np.array_equal(h, hw), mask
    gate_f16(ref, rdev, split_heads(base.spec, want[:, :3], hw[:3]), f"{name} mcs0 F12")


@pytest.mark.parametrize("name", ["a3_noh_3heads_u5", "a9_b5_u7"])
def test_y_layouts(name):
    # the Sionna resource grid and the split real / imag layout give the CGNN layout's outputs
    import torch
    full = base_case(name, 20)
    eng = engine_for(full)
    A = full.spec.num_rx_ant
    # B = 2: the first two slots
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[:2], np.float32)).cuda()  # noqa: E731
    y = full.y[:2]
    args = (torch.from_numpy(full.pe).cuda(), t(full.h_hat), t(full.active), t(full.mcs_mask))
    llr0, h0 = eng.forward(t(full.y), *args, num_it=full.num_it, precision="f32x")
    re, im = np.ascontiguousarray(y[..., :A]), np.ascontiguousarray(y[..., A:])
    grid = np.transpose(re + 1j * im, (0, 3, 2, 1))[:, None].astype(np.complex64)     # [B,1,A,14,F]
    llr1, h1 = eng.forward(torch.from_numpy(np.ascontiguousarray(grid)).cuda(), *args, num_it=full.num_it,
                           precision="f32x", y_layout="sionna")
    llr2, h2 = eng.forward(torch.from_numpy(re).cuda(), *args, num_it=full.num_it, precision="f32x",
                           y_layout="split", y_imag=torch.from_numpy(im).cuda())
    torch.cuda.synchronize()
    assert np.isfinite(llr0.cpu().numpy()).all()
    for llr, h in ((llr1, h1), (llr2, h2)):
        assert torch.equal(llr, llr0) and torch.equal(h, h0)
