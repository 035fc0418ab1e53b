"""The 3-D LMMSE channel estimator on the GPU (``nrx_chest_lmmse3``) against the numpy statement of
tests/chest3_ref.py, its estimate quality on a correlated channel and its leg of the evaluation
(needs an MI355X).

Cases (tests/chest3_ref.CASES; slots from the GPU generator with ``rx_corr = R_s``, seed 7,
cdm_group[u] = u % 2, 5 dB; R_s = rx_correlation(A, 0.9), or a random complex Hermitian PSD matrix):

    K1  U 2  A 4   F 24   DMRS (2, 11)     B 3              the bench model's geometry
    K2  U 1  A 2   F 13   DMRS (2,)        B 1              odd F, one DMRS symbol, 7 / 6 pilots, partial tiles
    K3  U 4  A 16  F 36   DMRS (2, 7, 11)  B 2, 2 active    nd = 3, N a full tile, inactive users written zero
    K4  U 2  A 3   F 132  DMRS (2, 11)     B 2              several M tiles, complex non-symmetric V_s, K = 66
    K5  U 2  A 1   F 12   DMRS (2, 11)     B 2              A = 1
    K6  U 2  A 4   F 24   DMRS (2, 3, 10, 11)  B 2          nd = 4: k_chest3_pilot<4>, k_chest3_expand<4, *>
    K7  U 2  A 4   F 24   DMRS (2,)        B 2              nd = 1, vector stores: k_chest3_expand<1, true>

Gate (the gate of tests/test_gpu_chest.py, unchanged).  e = max |gpu - ref| / max(1, |ref|) over
EVERY element against the float64 numpy application of the same f32-rounded tables
(chest3_ref.lmmse3_apply); floor = the same expression for the numpy float32 run against the float64
run; the test asserts e <= 8 * max(floor, 1e-6).  The tables come from chest.lmmse3_design on the
analytic covariance of chest_ref.model_covariance; the design itself is checked against the
brute-force Kronecker solve in tests/test_chest3_ref.py.

Figures of an MI355X run (as the tests print them: floor from numpy, e from the kernel; "R_s = I" is
max |lmmse3 - lmmse| / max(1, |lmmse|) between the two kernels, under its own case's gate):

    case  floor    e        gate     R_s = I
    K1    3.4e-7   2.8e-7   8.0e-6   5.6e-7
    K2    1.3e-7   1.6e-7   8.0e-6   1.2e-7
    K3    3.2e-7   5.5e-7   8.0e-6   7.5e-7
    K4    3.7e-7   3.5e-7   8.0e-6   8.3e-7
    K5    1.9e-7   2.7e-7   8.0e-6   3.6e-7
    K6    2.5e-7   2.6e-7   8.0e-6   3.6e-7
    K7    2.6e-7   1.8e-7   8.0e-6   3.0e-7

Into an output that is only 4-byte aligned (scalar stores): K1 e 2.8e-7, K3 5.5e-7, K6 2.6e-7.

Quality at 5 dB (U 2, A 4, F 48, covariance from 256 slots, 64 test slots), NMSE nearest / 2-D lmmse /
lmmse3: double_tdl_high 0.1490 / 0.0147 / 0.0072 (ratio 0.495; model value 0.49), double_tdl_low
0.1481 / 0.0146 / 0.0146 (ratio 1.001).  Evaluation at 10 dB, 2 PRB, 32 slots on double_tdl_high:
see the BER line the test prints; the default channel's run has the counts it had before the
channel option existed (NRX 2015 bit errors of 73728, lmmse_lmmse 1493).
"""
import functools

import numpy as np
import pytest

from tests import chest3_ref as R3
from tests import chest_ref as R
from tests import synth_chan_ref as C

pytestmark = pytest.mark.gpu

NAMES = list(R3.CASES)


def _rs(name):
    from neural_rx_amd.generator import rx_correlation
    _, A, _, _, _, _, kind = R3.CASES[name]
    return rx_correlation(A, 0.9) if kind == "corr" else C.random_psd(A, 31)


def _params(name, rx_corr="case"):
    from neural_rx_amd.generator import GenParams
    U, A, F, dmrs, _, na, _ = R3.CASES[name]
    return GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A, dmrs_symbols=dmrs,
                     cdm_group=tuple(u % 2 for u in range(U)), num_active=na, seed=R.SEED,
                     rx_corr=_rs(name) if rx_corr == "case" else rx_corr)


def _no(name):
    from neural_rx_amd.generator import ebno_to_no
    return ebno_to_no(R.EBNO_DB, len(R3.CASES[name][3]))


@functools.lru_cache(maxsize=None)
def _slots(name, batch=None):
    import torch
    from neural_rx_amd.generator import SlotGenerator
    sb = SlotGenerator(_params(name), want_h=True)(batch or R3.CASES[name][4], _no(name))
    torch.cuda.synchronize()
    g = {k: getattr(sb, k).cpu().numpy() for k in ("h_hat", "h", "active")}
    for a in g.values():
        a.setflags(write=False)
    return sb, g


@functools.lru_cache(maxsize=None)
def _design(name, identity=False):
    from neural_rx_amd.chest import lmmse3_design
    p = _params(name)
    R_s = np.eye(p.num_rx_ant) if identity else _rs(name)
    return lmmse3_design(*R.model_covariance(p.num_subcarriers), R_s, p)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(float64 oracle, float32 floor) of a case, computed once and shared read-only"""
    p = _params(name)
    _, g = _slots(name)
    run = lambda dt: R3.lmmse3_apply(g["h_hat"], g["active"], _design(name), p.dmrs_symbols, p.cdm_group,  # noqa: E731
                                     _no(name), dtype=dt)
    ref = run(np.float64)
    floor = float(np.max(np.abs(run(np.float32) - ref) / np.maximum(1.0, np.abs(ref))))
    ref.setflags(write=False)
    return ref, floor


def _run(name, sb=None, out=None, identity=False):
    import torch
    from neural_rx_amd.chest import ChannelEstimator
    est = ChannelEstimator("lmmse3", _params(name), tables=_design(name, identity))
    h = est(sb if sb is not None else _slots(name)[0], _no(name), out=out)
    torch.cuda.synchronize()
    return h


@pytest.mark.parametrize("name", NAMES)
def test_estimator_against_the_oracle(name):
    import torch
    _, g = _slots(name)
    ref, floor = _reference(name)
    out = torch.full(ref.shape, float("nan"), dtype=torch.float32, device="cuda")     # every element is written
    got = _run(name, out=out).cpu().numpy()
    assert np.isfinite(got).all()
    gate = 8.0 * max(floor, 1e-6)
    e = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
    print(f"{name} lmmse3: floor {floor:.2e}  e {e:.2e}  gate {gate:.2e}  max|ref| {np.abs(ref).max():.2f}")
    assert e <= gate, (name, e, gate)
    assert np.all(got[g["active"] <= 0] == 0.0)                                       # inactive planes are exactly 0
    if name == "K3":
        assert (g["active"] <= 0).any() and (g["active"] > 0).any()
    again = _run(name, out=torch.empty_like(out)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


@pytest.mark.parametrize("name", ["K1", "K3", "K4"])
def test_slot_0_alone_is_bit_identical(name):
    """the estimate of a slot does not depend on the batch it is in"""
    whole = _run(name).cpu().numpy()
    sb1, _ = _slots(name, batch=1)
    alone = _run(name, sb=sb1).cpu().numpy()
    assert np.array_equal(whole[:1].view(np.uint32), alone.view(np.uint32))


def test_only_the_own_pilots_are_read():
    import dataclasses
    import torch
    name = "K1"
    p = _params(name)
    sb, _ = _slots(name)
    masked = torch.full_like(sb.h_hat, float("nan"))
    for u in range(p.num_tx):
        for t in p.dmrs_symbols:
            masked[:, u, p.cdm_group[u]::2, t] = sb.h_hat[:, u, p.cdm_group[u]::2, t]
    got = _run(name, sb=dataclasses.replace(sb, h_hat=masked)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), _run(name).cpu().numpy().view(np.uint32))


def test_unaligned_output_takes_the_scalar_path():
    """K3 and K6 reach k_chest3_expand<3, false> and <4, false> this way only (A is a multiple of 4)"""
    import torch
    for name in ("K1", "K3", "K6"):
        ref, floor = _reference(name)
        buf = torch.full((ref.size + 1,), float("nan"), dtype=torch.float32, device="cuda")
        out = buf[1:].view(ref.shape)
        assert out.data_ptr() % 16 == 4
        got = _run(name, out=out).cpu().numpy()
        e = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
        print(f"{name} lmmse3 unaligned: floor {floor:.2e}  e {e:.2e}")
        assert e <= 8.0 * max(floor, 1e-6), (name, e)


@pytest.mark.parametrize("name", NAMES)
def test_identity_space_covariance_equals_the_2d_kernel(name):
    """R_s = I: within the same gate of nrx_chest_lmmse's output (floor: the numpy f32 run of the 3-D
    tables against its f64 run)"""
    from neural_rx_amd.chest import ChannelEstimator, lmmse_design
    import torch
    p = _params(name)
    sb, g = _slots(name)
    d3 = _design(name, identity=True)
    run = lambda dt: R3.lmmse3_apply(g["h_hat"], g["active"], d3, p.dmrs_symbols, p.cdm_group, _no(name), dtype=dt)  # noqa: E731
    ref = run(np.float64)
    floor = float(np.max(np.abs(run(np.float32) - ref) / np.maximum(1.0, np.abs(ref))))
    gate = 8.0 * max(floor, 1e-6)
    two = ChannelEstimator("lmmse", p, tables=lmmse_design(*R.model_covariance(p.num_subcarriers), p, _no(name)))
    h2 = two(sb, _no(name)).cpu().numpy()
    h3 = _run(name, identity=True).cpu().numpy()
    torch.cuda.synchronize()
    e = float(np.max(np.abs(h3 - h2) / np.maximum(1.0, np.abs(h2))))
    print(f"{name} R_s = I: |lmmse3 - lmmse| e {e:.2e}  gate {gate:.2e}")
    assert e <= gate, (name, e, gate)


# ---- estimate quality ----------------------------------------------------------------------------

def _nmse(est, sb):
    return float(((est - sb.h) ** 2).sum() / (sb.h ** 2).sum())


@functools.lru_cache(maxsize=None)
def _quality(scn):
    """NMSE of (nearest, 2-D lmmse, lmmse3) at 5 dB: U 2, A 4, F 48, covariance from 256 slots, 64 test slots"""
    import torch
    from neural_rx_amd.chest import ChannelEstimator, estimate_covariance
    from neural_rx_amd.generator import GenParams, SlotGenerator, ebno_to_no, scenario
    p = scenario(scn, GenParams(num_tx=2, num_subcarriers=48, num_rx_ant=4, seed=R.SEED))
    no = ebno_to_no(5.0, 2)
    gen = SlotGenerator(p, want_h=True)
    cov = estimate_covariance(gen, 256, 128)
    R_f, R_t = cov.matrices()
    sb = gen(64, no, slot_offset=0)
    e2 = _nmse(ChannelEstimator("lmmse", p, R_f=R_f, R_t=R_t)(sb, no), sb)
    e3 = _nmse(ChannelEstimator("lmmse3", p, R_f=R_f, R_t=R_t, R_s=cov.space())(sb, no), sb)
    nn = _nmse(sb.h_hat, sb)
    torch.cuda.synchronize()
    print(f"{scn} NMSE at 5 dB: nearest {nn:.4f}  2-D lmmse {e2:.4f}  lmmse3 {e3:.4f}  ratio {e3 / e2:.3f}")
    return nn, e2, e3


def test_3d_filter_beats_the_2d_filter_at_high_correlation():
    """model value of NMSE(lmmse3) / NMSE(2-D) at A = 4, alpha = 0.9, 5 dB: 0.49"""
    nn, e2, e3 = _quality("double_tdl_high")
    assert e3 < 0.75 * e2 < nn


def test_3d_filter_equals_the_2d_filter_without_correlation():
    nn, e2, e3 = _quality("double_tdl_low")
    assert abs(e3 - e2) <= 0.05 * e2 and e2 < nn


# ---- the evaluation --------------------------------------------------------------------------------

def test_evaluation_on_the_correlated_channel():
    """10 dB, 2 PRB, 32 slots on double_tdl_high: BER perfect CSI <= lmmse_lmmse with R_s <= lmmse_lmmse
    with the 2-D filter; the default run keeps its counts"""
    from neural_rx_amd import evaluate
    common = ["-config_name", "nrx_rt", "-num_tx_eval", "2", "-num_prbs", "2", "-ebno_db", "10", "-batch_size", "16",
              "-max_mc_iter", "2", "-num_cov_slots", "256"]
    d3 = evaluate.main(common + ["-channel", "double_tdl_high", "-baselines", "lmmse_lmmse", "perf_csi_lmmse"])
    d2 = evaluate.main(common + ["-channel", "double_tdl_high", "-chest_2d", "-baselines", "lmmse_lmmse"])
    assert d3["channel"] == d2["channel"] == "double_tdl_high" and d3["rx_corr"] == 0.9
    assert d3["counts"] == d2["counts"]                                    # the same slots, the same NRX
    ber = {"perf": d3["baselines"]["perf_csi_lmmse"]["ber"][0], "3d": d3["baselines"]["lmmse_lmmse"]["ber"][0],
           "2d": d2["baselines"]["lmmse_lmmse"]["ber"][0]}
    print("BER at 10 dB on double_tdl_high:", ber, " nrx", d3["ber"][0])
    assert d3["chest"] == "lmmse3" and d2["chest"] == "lmmse"
    assert ber["perf"] <= ber["3d"] <= ber["2d"]
    # the default channel: the counts of a run that names no channel at all
    base = evaluate.main(common + ["-baselines", "lmmse_lmmse"])
    iid = evaluate.main(common + ["-channel", "iid", "-baselines", "lmmse_lmmse"])
    assert set(base) == set(iid) and not {"channel", "rx_corr", "user_profiles"} & set(base)
    assert base["counts"] == iid["counts"] and base["baselines"]["lmmse_lmmse"]["counts"] == iid["baselines"]["lmmse_lmmse"]["counts"]
    assert base["counts"] != d3["counts"]
    # the counts this very run gave before the channel option existed (measured on that commit; they are
    # the BERs 0.0273 / 0.0203 of the tests/test_gpu_chest.py docstring)
    assert base["counts"] == [[2015, 73728, 63, 64]]
    assert base["baselines"]["lmmse_lmmse"]["counts"] == [[1493, 73728, 61, 64]]
    assert "chest" not in base                               # the default JSON keeps the keys it always had
