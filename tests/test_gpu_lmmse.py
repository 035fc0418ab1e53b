"""The LMMSE + max-log baseline detector on the GPU (``nrx_lmmse_detect``) against the numpy
reference of tests/lmmse_ref.py, and the baseline leg of the evaluation (needs an MI355X).

Cases (tests/lmmse_ref.CASES; seed 7, cdm_group[u] = u % 2, err_var = 0, slots from the GPU
generator with ``want_h=True``):

    C1  U 2  A 4   F 12  16-QAM   6 dB  B 3  the bench model's shape (LS and perfect CSI)
    C2  U 8  A 4   F 12  64-QAM  10 dB  B 2  U > A: rank-deficient Gram matrix (perfect CSI)
    C3  U 4  A 16  F 12  2/4/6 drawn, 2 active ports, 12 dB, B 4 (LS and perfect CSI)
    C4  U 1  A 2   F 13  QPSK     4 dB  B 1  scalar loads, odd width, partial wave, one DMRS symbol
    C5  U 2  A 4   F 12  16-QAM   8 dB  B 5  840 REs: grid tail of a 256-thread block
    C6  U 3  A 4   F 12  16-QAM   8 dB  B 2  non-power-of-two U (perfect CSI)
    C7  U 5  A 8   F 12  16-QAM   8 dB  B 2  k_lmmse<5, true>   (C7..C13: perfect CSI)
    C8  U 6  A 8   F 12  64-QAM  12 dB  B 2  k_lmmse<6, true>
    C9  U 7  A 8   F 12  QPSK     2 dB  B 2  k_lmmse<7, true>: two antennas per step at a U other than 8
    C10 U 5  A 6   F 12  16-QAM   8 dB  B 2  k_lmmse<5, false>
    C11 U 6  A 10  F 12  16-QAM   8 dB  B 2  k_lmmse<6, false>
    C12 U 7  A 10  F 12  64-QAM  12 dB  B 2  k_lmmse<7, false>: scalar loads at U >= 7
    C13 U 1  A 4   F 12  QPSK     4 dB  B 2  k_lmmse<1, true> (C4 is its scalar twin)

tests/dispatch_cases.py names, for every ``case`` of ``launch_lmmse`` and both values of ``vec``, the case that
runs it; U = 2, 3, 4, 8 reach the scalar kernels through the unaligned test.

Gate.  e = max |llr_gpu - llr_ref| / max(1, |llr_ref|) against the float64 reference; floor = the
same expression for the reference's own float32 run against its float64 run (reference against
reference, never the kernel); the test asserts e <= 8 * max(floor, 1e-5).  The 8 covers the
kernel's FMA contraction and its unpivoted LDL^H order against LAPACK's inverse; the 1e-5 (about
170 f32 ulps) is there because C4's floor is only a few ulps.  Signs must agree wherever |llr_ref|
exceeds the element's gate; at most 1 % of the active data elements may be left out, and the GPU
error counters must equal the reference's to within the number left out.

Figures of an MI355X run (as the test prints them: floor from numpy, e from the kernel, both on
the GPU generator's slots):

    case  csi      floor    e        gate     left out
    C1    ls       7.9e-6   8.5e-6   8.0e-5   0
    C1    perfect  6.2e-6   6.1e-6   8.0e-5   0
    C2    perfect  5.1e-5   5.6e-5   4.1e-4   24 (0.17 %)
    C3    ls       5.7e-6   2.1e-5   8.0e-5   0
    C3    perfect  3.5e-6   3.8e-6   8.0e-5   0
    C4    ls       7.1e-7   8.7e-7   8.0e-5   0
    C4    perfect  3.8e-7   3.1e-7   8.0e-5   0
    C5    ls       1.1e-5   1.3e-5   8.6e-5   0
    C5    perfect  2.0e-5   1.1e-5   1.6e-4   0
    C6    perfect  1.0e-5   8.5e-6   8.0e-5   0
    C7    perfect  1.8e-5   1.5e-5   1.5e-4   0
    C8    perfect  5.5e-5   5.9e-5   4.4e-4   0
    C9    perfect  1.8e-5   1.3e-5   1.4e-4   0
    C10   perfect  1.3e-5   1.3e-5   1.0e-4   0
    C11   perfect  2.5e-5   2.1e-5   2.0e-4   0
    C12   perfect  4.8e-5   6.3e-5   3.8e-4   0
    C13   perfect  4.1e-7   3.3e-7   8.0e-5   0
    unaligned (scalar loads and stores), perfect CSI:
    C1             6.2e-6   6.1e-6   8.0e-5   0
    C6             1.0e-5   9.6e-6   8.0e-5   0
    C3             3.5e-6   3.4e-6   8.0e-5   0
    C2             5.1e-5   5.2e-5   4.1e-4   24 (0.17 %)

The GPU bit-error counts equal the reference's (and the table's) on every case.  min mu over the
active RE-users is >= 0.17 on every case (asserted >= 1e-3), far from the mu < 1e-6 rule.
"""
import functools

import numpy as np
import pytest

from oracle import synth_ref as S
from tests import lmmse_ref as R

pytestmark = pytest.mark.gpu

CASE_CSI = [(n, c) for n in R.CASES for c in R.CASES[n][9]]


def _params(name):
    from neural_rx_amd.generator import GenParams
    s = R.case_spec(name)
    return GenParams(num_tx=s.num_tx, num_subcarriers=s.num_subcarriers, num_rx_ant=s.num_rx_ant,
                     dmrs_symbols=s.dmrs_symbols, cdm_group=s.cdm_group, mcs_bits=s.mcs_bits,
                     mcs_of_user=s.mcs_of_user, num_active=s.num_active, seed=s.seed), s.no


@functools.lru_cache(maxsize=None)
def _slots(name):
    """(device SlotBatch, host copies) of a case, generated once"""
    import torch
    from neural_rx_amd.generator import SlotGenerator
    p, no = _params(name)
    sb = SlotGenerator(p, want_h=True)(R.CASES[name][6], no)
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
def _reference(name, csi, err_var=0.0):
    """float64 LLRs, mu, the float32 floor and the mask of active data elements -- computed once
    per case and shared (read-only) by the tests"""
    p, no = _params(name)
    _, g = _slots(name)
    h = g["h_hat"] if csi == "ls" else g["h"]
    args = (g["y"], h, g["active"], g["mcs"], p.mcs_bits, no, p.dmrs_symbols)
    ref, mu = R.lmmse_detect(*args, err_var=err_var, return_mu=True)
    r32 = R.lmmse_detect(*args, err_var=err_var, dtype=np.float32)
    floor = float(np.max(np.abs(r32 - ref) / np.maximum(1.0, np.abs(ref))))
    used = _used(p, g["active"], g["mcs"])
    for a in (ref, mu, used):
        a.setflags(write=False)
    return ref, mu, floor, used


def _detect(name, csi, err_var=0.0, out=None):
    import torch
    from neural_rx_amd.baseline import LMMSEDetector
    p, no = _params(name)
    sb, _ = _slots(name)
    llr = LMMSEDetector()(sb.y, sb.h_hat if csi == "ls" else sb.h, sb.active, sb.mcs, p.mcs_bits, no,
                          p.dmrs_symbols, err_var=err_var, out=out)
    torch.cuda.synchronize()
    return llr


def _gate_check(tag, llr, ref, floor, used):
    """accuracy + sign agreement; returns the number of elements left out of the sign check"""
    gate = 8.0 * max(floor, 1e-5)
    e = float(np.max(np.abs(llr - ref) / np.maximum(1.0, np.abs(ref))))
    left_out = used & (np.abs(ref) <= gate * np.maximum(1.0, np.abs(ref)))
    share = left_out.sum() / used.sum()
    print(f"{tag}: floor {floor:.2e}  e {e:.2e}  gate {gate:.2e}  left out {int(left_out.sum())} "
          f"({100 * share:.3f} %)  max|llr| {np.abs(ref).max():.1f}")
    assert np.isfinite(llr).all()
    assert e <= gate, (tag, e, gate)
    chk = used & ~left_out
    assert np.array_equal(np.sign(llr[chk]), np.sign(ref[chk])), tag
    assert share <= 0.01, (tag, share)
    return int(left_out.sum())


@pytest.mark.parametrize("name,csi", CASE_CSI)
def test_case(name, csi):
    import torch
    from neural_rx_amd.generator import count_errors
    p, no = _params(name)
    sb, g = _slots(name)
    ref, mu, floor, used = _reference(name, csi)
    # conditioning: no case sits on the mu < 1e-6 rule
    act_re = (g["active"] > 0)[:, :, None, None] & used[..., 0]
    assert mu[act_re].min() >= 1e-3
    # every element is written: the buffer starts as NaN
    out = torch.full(ref.shape, float("nan"), dtype=torch.float32, device="cuda")
    llr_t = _detect(name, csi, out=out)
    llr = llr_t.cpu().numpy()
    left_out = _gate_check(f"{name} {csi}", llr[0], ref[0], floor, used)
    # exact zeros: inactive users, DMRS symbols, entries k >= bits
    assert np.all(llr[0][~used] == 0.0)
    # determinism: a second call into a fresh buffer is bit-identical
    again = _detect(name, csi).cpu().numpy()
    assert np.array_equal(llr.view(np.uint32), again.view(np.uint32))
    # counters on the GPU LLRs against the reference's
    cnt = count_errors(llr_t, sb.bits, sb.active, sb.mcs, p.mcs_bits, p.dmrs_symbols).cpu().numpy().sum(0)
    rc = S.count_errors(ref, g["bits"], g["mcs"], p.mcs_bits, g["active"], p.dmrs_symbols).sum(0)
    print(f"{name} {csi}: bit errors gpu {cnt[0]} ref {rc[0]} of {rc[1]} (table {R.CASES[name][9][csi]})")
    assert cnt[1] == rc[1] == R.CASES[name][9][csi][1] and cnt[3] == rc[3]
    assert abs(int(cnt[0]) - int(rc[0])) <= left_out


@pytest.mark.parametrize("bs", [8, 5])
def test_wider_and_odd_bits_stride(bs):
    """bits_stride > max(mcs_bits): the generic store path; the extra entries are written 0"""
    import torch
    ref, _, floor, used = _reference("C1", "ls")
    out = torch.full((1,) + ref.shape[1:5] + (bs,), float("nan"), dtype=torch.float32, device="cuda")
    llr = _detect("C1", "ls", out=out).cpu().numpy()
    _gate_check(f"C1 ls stride {bs}", llr[0][..., :4], ref[0], floor, used)
    assert np.all(llr[..., 4:] == 0.0)


def test_unaligned_tensors_take_the_scalar_paths():
    """y, h and llr that are only 4-byte aligned: scalar loads and stores, same LLRs.  C6, C3 and C2 have
    A % 4 == 0, so this is what takes U = 3, 4 and 8 to k_lmmse<U, false>."""
    import torch
    from neural_rx_amd.baseline import LMMSEDetector

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    for name in ("C1", "C6", "C3", "C2"):
        p, no = _params(name)
        sb, _ = _slots(name)
        ref, _, floor, used = _reference(name, "perfect")
        out = shifted(torch.full(ref.shape, float("nan"), dtype=torch.float32, device="cuda"))
        llr = LMMSEDetector()(shifted(sb.y), shifted(sb.h), sb.active, sb.mcs, p.mcs_bits, no, p.dmrs_symbols, out=out)
        torch.cuda.synchronize()
        _gate_check(f"{name} perfect unaligned", llr.cpu().numpy()[0], ref[0], floor, used)


def test_all_zero_channel():
    """G = s I, mu = 0 < 1e-6: every LLR finite and exactly 0"""
    import torch
    from neural_rx_amd.baseline import LMMSEDetector
    y = torch.randn((2, 12, 14, 8), device="cuda")
    h = torch.zeros((2, 2, 12, 14, 8), device="cuda")
    out = torch.full((1, 2, 2, 12, 14, 4), float("nan"), device="cuda")
    llr = LMMSEDetector()(y, h, torch.ones((2, 2), device="cuda"), None, (4,), 0.1, (2, 11), out=out)
    torch.cuda.synchronize()
    assert np.all(llr.cpu().numpy() == 0.0)


def _baseline_counts(name, system):
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.generator import count_errors
    p, no = _params(name)
    sb, _ = _slots(name)
    llr = BaselineReceiver(system, p)(sb, no)
    return count_errors(llr, sb.bits, sb.active, sb.mcs, p.mcs_bits, p.dmrs_symbols).cpu().numpy().sum(0)


@pytest.mark.parametrize("name", ["C1", "C5"])
def test_perfect_csi_beats_ls_on_the_same_slots(name):
    ls = _baseline_counts(name, "baseline_lsnn_lmmse")
    pc = _baseline_counts(name, "baseline_perf_csi_lmmse")
    print(f"{name}: bit errors perfect CSI {pc[0]}  LS {ls[0]}  of {ls[1]}")
    assert pc[1] == ls[1] == R.CASES[name][9]["ls"][1]
    assert pc[0] < ls[0]


# ---- the evaluation's baseline leg ---------------------------------------------------------

EVAL_B, EVAL_ITERS, EVAL_EBNO = 4, 2, 6.0


@pytest.mark.parametrize("system", ["baseline_lsnn_lmmse", "baseline_perf_csi_lmmse"])
def test_sim_ber_baseline_counts(system):
    """nrx_rt at 1 PRB, B = 4, one point, two iterations: the summed counters are the reference's
    on the global slot offsets it * B (rank 0 of 1)"""
    import torch
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.evaluate import sim_ber_baseline
    from neural_rx_amd.generator import GenParams, SlotGenerator, ebno_to_no
    p = GenParams.from_config("nrx_rt", num_prbs=1, seed=4)
    gen = SlotGenerator(p, want_h=True)
    rx = BaselineReceiver(system, p)
    r = sim_ber_baseline(rx, gen, [EVAL_EBNO], batch_size=EVAL_B, max_mc_iter=EVAL_ITERS,
                         num_target_block_errors=10**9, early_stop=False)
    assert r.mc_iters == [EVAL_ITERS] and r.slots == EVAL_B * EVAL_ITERS
    no = ebno_to_no(EVAL_EBNO, len(p.dmrs_symbols))
    ref_cnt, left_out = np.zeros(4, np.int64), 0
    for it in range(EVAL_ITERS):
        sb = gen(EVAL_B, no, slot_offset=it * EVAL_B)
        torch.cuda.synchronize()
        g = {k: getattr(sb, k).cpu().numpy() for k in ("y", "h", "h_hat", "active", "mcs", "bits")}
        args = (g["y"], g["h"] if rx.perfect_csi else g["h_hat"], g["active"], g["mcs"], p.mcs_bits, no,
                p.dmrs_symbols)
        ref = R.lmmse_detect(*args, err_var=rx.err_var(no))
        r32 = R.lmmse_detect(*args, err_var=rx.err_var(no), dtype=np.float32)
        gate = 8.0 * max(float(np.max(np.abs(r32 - ref) / np.maximum(1.0, np.abs(ref)))), 1e-5)
        left_out += int((_used(p, g["active"], g["mcs"]) & (np.abs(ref[0]) <= gate)).sum())
        ref_cnt += S.count_errors(ref, g["bits"], g["mcs"], p.mcs_bits, g["active"], p.dmrs_symbols).sum(0)
    print(f"{system}: counts {r.counts[0]}  reference {ref_cnt.tolist()}  left out {left_out}")
    assert r.counts[0][1] == ref_cnt[1] and r.counts[0][3] == ref_cnt[3] == EVAL_B * EVAL_ITERS * 2
    assert abs(r.counts[0][0] - ref_cnt[0]) <= left_out
    assert abs(r.counts[0][2] - ref_cnt[2]) <= left_out
    assert rx.err_var(no) == (0.0 if rx.perfect_csi else no)          # two active ports: 2 no / 2


def test_evaluate_cli_baselines(capsys):
    from neural_rx_amd import evaluate
    argv = ["-config_name", "nrx_rt", "-num_prbs", "1", "-ebno_db", "6", "-batch_size", "4", "-max_mc_iter", "2"]
    plain = evaluate.main(argv)
    assert set(plain) == {"ebno_db", "ber", "bler", "counts", "mc_iters", "seconds", "slots", "config",
                          "num_tx_eval", "dmrs_symbols", "world", "slots_per_s"}
    assert "nrx  EbNo" not in capsys.readouterr().out
    both = evaluate.main(argv + ["-baselines", "lsnn_lmmse", "perf_csi_lmmse"])
    assert set(both) == set(plain) | {"baselines"}
    assert set(both["baselines"]) == {"lsnn_lmmse", "perf_csi_lmmse"}
    assert both["counts"] == plain["counts"]                          # the NRX leg is unchanged
    for r in both["baselines"].values():
        assert set(r) == {"ebno_db", "ber", "bler", "counts", "mc_iters", "seconds", "slots"}
        assert r["counts"][0][1] == plain["counts"][0][1]             # paired: the same bits
    text = capsys.readouterr().out
    assert "nrx  EbNo" in text and "lsnn_lmmse  EbNo" in text and "perf_csi_lmmse  EbNo" in text
    assert "pilot-contaminated" not in text                           # one port per CDM group
