"""The K-best detector on the GPU (``nrx_kbest_detect``) against the numpy references of
tests/kbest_ref.py, and the K-best leg of the evaluation (needs an MI355X).

Cases (tests/kbest_ref.CASES; seed 7, F 12, DMRS (2, 11), cdm_group[u] = u % 2, perfect CSI,
err_var = 0, k = 64, llr_clip = 20, slots from the GPU generator with ``want_h=True``):

    K1  U 1  A 2   64-QAM   8 dB  B 2  exhaustive (64 leaves): against max-log ML
    K2  U 3  A 4   QPSK     4 dB  B 2  exhaustive (64 leaves): against max-log ML
    K3  U 4  A 4   16-QAM  10 dB  B 3  pruned (65 536 leaves)
    K4  U 2  A 4   64-QAM  14 dB  B 3  pruned (4096 leaves)
    K5  U 8  A 8   QPSK    -2 dB  B 2  pruned, 16 levels
    K6  U 4  A 16  2/4/6 drawn, 2 active ports, 0 dB, B 4: mixed L, inactive users
    K7  U 5  A 8   QPSK     0 dB  B 2  pruned, 10 levels: k_kbest_gram<5, true>
    K8  U 6  A 8   QPSK     0 dB  B 2  pruned, 12 levels: k_kbest_gram<6, true>
    K9  U 7  A 8   QPSK     0 dB  B 2  pruned, 14 levels: k_kbest_gram<7, true>
    K10 U 5  A 5   16-QAM  10 dB  B 2  pruned; odd A: k_kbest_gram<5, false>
    K11 U 2  A 4   QPSK     2 dB  B 456  exhaustive (16 leaves); 65 664 data REs on a search grid of 65 536
                                          waves: 128 waves take a second RE

tests/dispatch_cases.py names, for every ``case`` of ``launch_kbest`` and both values of ``vec``, the case that
runs it; the scalar Gram kernels of U = 1, 2, 3, 4, 6, 7, 8 run through the unaligned test.

Gate.  e = max |llr_gpu - llr_ref| / max(1, |llr_ref|) against the float64 reference (ML for K1 and
K2, kbest_ref for the rest); floor = the same expression for kbest_ref's own float32 run against
its float64 run (reference against reference, never the kernel); gate = 8 * max(floor, 1e-5).  On
the exhaustive cases every element must pass.  On the pruned cases an element above the gate is a
survivor-set flip caused by a different rounding order (the kernel builds the Gram matrix antenna
by antenna and contracts to FMAs); those are left out, at most 0.5 % of the used elements (active
user, data symbol, k < bits).  Signs must agree wherever |ref| exceeds the gate and the element
was not left out, and the GPU bit-error count may differ from the reference's by no more than the
number left out (exhaustive cases: the number of elements with |ref| below the gate).

The test prints floor, e, gate and the left-out count per case.  Figures of an MI355X run (floor
from numpy, e from the kernel, both on the GPU generator's slots; DESIGN.md section 9 has the
same table):

    case          floor    e        gate     left out  bit errors gpu = ref
    K1            1.4e-6   1.4e-6   8.0e-5   0         299 / 1728
    K2            2.0e-6   1.6e-6   8.0e-5   0           9 / 1728
    K3            2.9e-5   2.8e-5   2.3e-4   0         156 / 6912
    K4            1.4e-5   1.4e-5   1.1e-4   0          66 / 5184
    K5            4.8e-6   6.1e-6   8.0e-5   0         107 / 4608
    K6            5.3e-6   5.9e-6   8.0e-5   0         103 / 4032
    K7            2.5e-6   1.7e-6   8.0e-5   0           5 / 2880
    K8            2.3e-6   3.7e-6   8.0e-5   0           5 / 3456
    K9            3.8e-6   5.8e-6   8.0e-5   0           7 / 4032
    K10           2.7e-5   2.9e-5   2.2e-4   0          30 / 5760
    K11           4.3e-6   4.0e-6   8.0e-5   0        4376 / 262656
    K3 k = 1      0        0        8.0e-5   0
    K3 k = 16     2.9e-5   2.8e-5   2.3e-4   0
    K3 unaligned  2.9e-5   5.9e-5   2.3e-4   0
    K1 unaligned  1.4e-6   1.4e-6   8.0e-5   0
    K4 unaligned  1.4e-5   1.9e-5   1.1e-4   0
    K2 unaligned  2.0e-6   1.6e-6   8.0e-5   0
    K8 unaligned  2.3e-6   3.8e-6   8.0e-5   0
    K9 unaligned  3.8e-6   5.8e-6   8.0e-5   0
    K5 unaligned  4.8e-6   6.1e-6   8.0e-5   0
"""
import functools

import numpy as np
import pytest

from oracle import synth_ref as S
from tests import kbest_ref as K

pytestmark = pytest.mark.gpu

MAX_LEFT_OUT = 0.005


def _params(name):
    from neural_rx_amd.generator import GenParams
    s = K.case_spec(name)
    return GenParams(num_tx=s.num_tx, num_subcarriers=s.num_subcarriers, num_rx_ant=s.num_rx_ant,
                     dmrs_symbols=s.dmrs_symbols, cdm_group=s.cdm_group, mcs_bits=s.mcs_bits,
                     mcs_of_user=s.mcs_of_user, num_active=s.num_active, seed=s.seed), s.no


@functools.lru_cache(maxsize=None)
def _slots(name):
    """(device SlotBatch, host copies) of a case, generated once"""
    import torch
    from neural_rx_amd.generator import SlotGenerator
    p, no = _params(name)
    sb = SlotGenerator(p, want_h=True)(K.CASES[name][6], no)
    torch.cuda.synchronize()
    return sb, {k: v.cpu().numpy() for k, v in vars(sb).items() if v is not None}


def _used(p, active, mcs):
    """[B, U, F, T, bits_max] mask of the LLRs that carry a bit: active user, data symbol, k < bits"""
    data = np.ones(14, bool)
    data[list(p.dmrs_symbols)] = False
    nbits = np.array(p.mcs_bits)[mcs]
    m = (active > 0)[:, :, None, None, None] & data[None, None, None, :, None] \
        & (np.arange(p.bits_max)[None, None, None, None, :] < nbits[:, :, None, None, None])
    return np.broadcast_to(m, active.shape + (p.num_subcarriers, 14, p.bits_max)).copy()


@functools.lru_cache(maxsize=None)
def _reference(name, k=64):
    """(float64 reference LLRs, float32 floor of kbest_ref, mask of used elements, min pivot ratio)
    -- computed once per (case, k) and shared read-only.  The reference is max-log ML on the
    exhaustive cases at k = 64 and kbest_ref otherwise."""
    p, no = _params(name)
    _, g = _slots(name)
    args = (g["y"], g["h"], g["active"], g["mcs"], p.mcs_bits, no, p.dmrs_symbols)
    r64, ratio = K.kbest_detect(*args, k=k, return_pivot=True)
    r32 = K.kbest_detect(*args, k=k, dtype=np.float32)
    floor = float(np.max(np.abs(r32 - r64) / np.maximum(1.0, np.abs(r64))))
    ref = K.ml_detect(*args) if K.CASES[name][9] and k == 64 else r64
    used = _used(p, g["active"], g["mcs"])
    for a in (ref, used):
        a.setflags(write=False)
    return ref, floor, used, ratio


def _detect(name, k=64, out=None, **kw):
    import torch
    from neural_rx_amd.kbest import KBestDetector
    p, no = _params(name)
    sb, _ = _slots(name)
    llr = KBestDetector()(sb.y, sb.h, sb.active, sb.mcs, p.mcs_bits, no, p.dmrs_symbols, k=k, out=out, **kw)
    torch.cuda.synchronize()
    return llr


def _gate_check(tag, llr, ref, floor, used, exhaustive):
    """accuracy + sign agreement; returns the number of elements a bit-error count may differ by"""
    gate = 8.0 * max(floor, 1e-5)
    err = np.abs(llr - ref) / np.maximum(1.0, np.abs(ref))
    flips = err > gate
    e = float(err[~flips].max()) if not exhaustive else float(err.max())
    share = flips.sum() / used.sum()
    print(f"{tag}: floor {floor:.2e}  e {e:.2e}  gate {gate:.2e}  left out {int(flips.sum())} "
          f"({100 * share:.3f} %)  worst {float(err.max()):.2e}")
    assert np.isfinite(llr).all()
    assert np.all(llr[~used] == 0.0)                      # inactive users, DMRS symbols, k >= bits
    assert not flips[~used].any()
    if exhaustive:
        assert e <= gate, (tag, e, gate)
    else:
        assert share <= MAX_LEFT_OUT, (tag, share)
    small = used & (np.abs(ref) <= gate)
    chk = used & ~flips & ~small
    assert np.array_equal(np.sign(llr[chk]), np.sign(ref[chk])), tag
    return int(small.sum()) if exhaustive else int(flips.sum())


@pytest.mark.parametrize("name", list(K.CASES))
def test_case(name):
    import torch
    from neural_rx_amd.generator import count_errors
    p, no = _params(name)
    sb, g = _slots(name)
    ref, floor, used, ratio = _reference(name)
    assert ratio >= 1e-3                                   # no case sits on the pivot rule
    # every element is written: the buffer starts as NaN
    out = torch.full(ref.shape, float("nan"), dtype=torch.float32, device="cuda")
    llr_t = _detect(name, out=out)
    llr = llr_t.cpu().numpy()
    slack = _gate_check(name, llr[0], ref[0], floor, used, K.CASES[name][9])
    # determinism: a second call into a fresh buffer is bit-identical
    again = _detect(name).cpu().numpy()
    assert np.array_equal(llr.view(np.uint32), again.view(np.uint32))
    # counters on the GPU LLRs against the reference's
    cnt = count_errors(llr_t, sb.bits, sb.active, sb.mcs, p.mcs_bits, p.dmrs_symbols).cpu().numpy().sum(0)
    rc = S.count_errors(ref, g["bits"], g["mcs"], p.mcs_bits, g["active"], p.dmrs_symbols).sum(0)
    print(f"{name}: bit errors gpu {cnt[0]} ref {rc[0]} of {rc[1]} (table {K.CASES[name][10]})")
    assert cnt[1] == rc[1] == K.CASES[name][10][2] and cnt[3] == rc[3]
    assert abs(int(cnt[0]) - int(rc[0])) <= slack


@pytest.mark.parametrize("name", ["K3", "K5"])
def test_kbest_beats_lmmse_on_the_same_slots(name):
    import torch
    from neural_rx_amd.baseline import LMMSEDetector
    from neural_rx_amd.generator import count_errors
    p, no = _params(name)
    sb, _ = _slots(name)
    kb = _detect(name)
    lm = LMMSEDetector()(sb.y, sb.h, sb.active, sb.mcs, p.mcs_bits, no, p.dmrs_symbols)
    torch.cuda.synchronize()
    ck, cl = (count_errors(x, sb.bits, sb.active, sb.mcs, p.mcs_bits, p.dmrs_symbols).cpu().numpy().sum(0)
              for x in (kb, lm))
    print(f"{name}: bit errors K-best {ck[0]}  LMMSE {cl[0]}  of {ck[1]}")
    assert ck[1] == cl[1] == K.CASES[name][10][2]
    assert ck[0] < cl[0]


@pytest.mark.parametrize("k", [1, 16])
def test_partial_wave_k(k):
    """k < 64 on K3: the survivor list fills a part of the wave"""
    ref, floor, used, _ = _reference("K3", k)
    llr = _detect("K3", k=k).cpu().numpy()
    _gate_check(f"K3 k {k}", llr[0], ref[0], floor, used, False)


@pytest.mark.parametrize("bs", [6, 7])
def test_wider_bits_stride(bs):
    """bits_stride > max(mcs_bits) on a 4-bit case: the extra entries are written 0"""
    import torch
    ref, floor, used, _ = _reference("K3")
    out = torch.full((1,) + ref.shape[1:5] + (bs,), float("nan"), dtype=torch.float32, device="cuda")
    llr = _detect("K3", out=out).cpu().numpy()
    _gate_check(f"K3 stride {bs}", llr[0][..., :4], ref[0], floor, used, False)
    assert np.all(llr[..., 4:] == 0.0)


def test_unaligned_tensors_take_the_scalar_paths():
    """y, h and llr that are only 4-byte aligned: scalar loads and stores, same LLRs.  Every one of these
    cases has an even A, so this is what takes U = 1, 2, 3, 4, 6, 7 and 8 to k_kbest_gram<U, false>."""
    import torch
    from neural_rx_amd.kbest import KBestDetector

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    for name in ("K3", "K1", "K4", "K2", "K8", "K9", "K5"):
        p, no = _params(name)
        sb, _ = _slots(name)
        ref, floor, used, _ = _reference(name)
        out = shifted(torch.full(ref.shape, float("nan"), dtype=torch.float32, device="cuda"))
        llr = KBestDetector()(shifted(sb.y), shifted(sb.h), sb.active, sb.mcs, p.mcs_bits, no, p.dmrs_symbols, out=out)
        torch.cuda.synchronize()
        _gate_check(f"{name} unaligned", llr.cpu().numpy()[0], ref[0], floor, used, K.CASES[name][9])


def test_batch_split_is_bit_identical():
    """B = 3 in one call equals its slots in calls of 1 and 2, bit for bit"""
    import torch
    from neural_rx_amd.kbest import KBestDetector
    p, no = _params("K3")
    sb, _ = _slots("K3")
    whole = _detect("K3").cpu().numpy()
    det = KBestDetector()
    parts = []
    for lo, hi in ((0, 1), (1, 3)):
        parts.append(det(sb.y[lo:hi], sb.h[lo:hi], sb.active[lo:hi], sb.mcs[lo:hi], p.mcs_bits, no,
                         p.dmrs_symbols).clone())
    torch.cuda.synchronize()
    split = torch.cat(parts, 1).cpu().numpy()
    assert np.array_equal(whole.view(np.uint32), split.view(np.uint32))


def test_all_zero_channel():
    """every pivot is 0 <= 1e-6 G_ii: every LLR finite and exactly 0"""
    import torch
    from neural_rx_amd.kbest import KBestDetector
    y = torch.randn((2, 12, 14, 8), device="cuda")
    h = torch.zeros((2, 2, 12, 14, 8), device="cuda")
    out = torch.full((1, 2, 2, 12, 14, 4), float("nan"), device="cuda")
    llr = KBestDetector()(y, h, torch.ones((2, 2), device="cuda"), None, (4,), 0.1, (2, 11), out=out)
    torch.cuda.synchronize()
    assert np.all(llr.cpu().numpy() == 0.0)


# ---- the evaluation's K-best leg ----------------------------------------------------------

EVAL_B, EVAL_ITERS, EVAL_EBNO = 4, 2, (2.0, 6.0)


@functools.lru_cache(maxsize=None)
def _eval_setup():
    from neural_rx_amd.chest import estimate_covariance
    from neural_rx_amd.generator import GenParams, SlotGenerator
    p = GenParams.from_config("nrx_rt", num_prbs=2, seed=4)
    gen = SlotGenerator(p, want_h=True)
    R_f, R_t = estimate_covariance(gen, 32, 16).matrices()
    return p, gen, R_f, R_t


@pytest.mark.parametrize("system", ["baseline_lmmse_kbest", "baseline_perf_csi_kbest"])
def test_sim_ber_baseline_counts(system):
    """nrx_rt at 2 PRB, B = 4, two points, two iterations: the counters are those of a direct
    estimator + detector + counter loop on the same slot offsets, and the bit totals are the LMMSE
    baseline's (the slots are paired)"""
    import torch
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.chest import ChannelEstimator, EstimatorBaselineReceiver
    from neural_rx_amd.evaluate import sim_ber_baseline
    from neural_rx_amd.generator import count_errors, ebno_to_no
    from neural_rx_amd.kbest import KBestBaselineReceiver, KBestDetector
    p, gen, R_f, R_t = _eval_setup()
    rx = KBestBaselineReceiver(system, p, R_f=R_f, R_t=R_t)
    kw = dict(batch_size=EVAL_B, max_mc_iter=EVAL_ITERS, num_target_block_errors=10**9, early_stop=False)
    r = sim_ber_baseline(rx, gen, list(EVAL_EBNO), **kw)
    assert r.mc_iters == [EVAL_ITERS] * 2 and r.slots == EVAL_B * EVAL_ITERS * 2
    det = KBestDetector()
    est = ChannelEstimator("lmmse", p, R_f=R_f, R_t=R_t)
    twin = EstimatorBaselineReceiver("baseline_lmmse_lmmse", p, R_f=R_f, R_t=R_t)
    for k, ebno in enumerate(EVAL_EBNO):
        no = ebno_to_no(ebno, len(p.dmrs_symbols))
        ev = 0.0 if rx.perfect_csi else twin.err_var(no)
        assert rx.err_var(no) == ev and (ev > 0.0) == (not rx.perfect_csi)
        total = np.zeros(4, np.int64)
        for it in range(EVAL_ITERS):
            sb = gen(EVAL_B, no, slot_offset=(k * EVAL_ITERS + it) * EVAL_B)
            h = sb.h if rx.perfect_csi else est(sb, no)
            llr = det(sb.y, h, sb.active, sb.mcs, p.mcs_bits, no, p.dmrs_symbols, err_var=ev)
            total += count_errors(llr, sb.bits, sb.active, sb.mcs, p.mcs_bits, p.dmrs_symbols).cpu().numpy().sum(0)
        torch.cuda.synchronize()
        print(f"{system} {ebno} dB: counts {r.counts[k]}  direct {total.tolist()}")
        assert r.counts[k] == total.tolist()
    lm = sim_ber_baseline(BaselineReceiver("baseline_perf_csi_lmmse", p), gen, list(EVAL_EBNO), **kw)
    assert [c[1] for c in r.counts] == [c[1] for c in lm.counts]
    assert [c[3] for c in r.counts] == [c[3] for c in lm.counts]


def test_evaluate_cli_kbest(capsys):
    from neural_rx_amd import evaluate
    argv = ["-config_name", "nrx_rt", "-num_prbs", "1", "-ebno_db", "6", "-batch_size", "4", "-max_mc_iter", "2",
            "-num_cov_slots", "16"]
    d = evaluate.main(argv + ["-baselines", "perf_csi_lmmse", "perf_csi_kbest", "lmmse_kbest", "-kbest_k", "32"])
    assert set(d["baselines"]) == {"perf_csi_lmmse", "perf_csi_kbest", "lmmse_kbest"}
    assert d["num_cov_slots"] == 16                                   # the covariance path ran
    for r in d["baselines"].values():
        assert set(r) == {"ebno_db", "ber", "bler", "counts", "mc_iters", "seconds", "slots"}
        assert r["counts"][0][1] == d["counts"][0][1]                 # paired: the same bits
    text = capsys.readouterr().out
    assert "perf_csi_kbest  EbNo" in text and "lmmse_kbest  EbNo" in text
