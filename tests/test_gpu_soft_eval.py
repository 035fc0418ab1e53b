"""The soft metrics inside the Monte-Carlo loop (``evaluate.sim_ber`` / ``sim_ber_baseline`` with
``soft=``) for the neural receiver and two baselines (needs an MI355X).

Shape: nrx_rt weights, 4 PRB, 2 users, B = 8, Eb/N0 0 and 12 dB, two Monte-Carlo batches per point.

The expected values come from replaying the loop's slots (same generator, same offsets) through the
same receiver, copying its LLRs (and channel estimate) to the host and applying the numpy reference
of tests/softmetrics_ref.py: BMI within 1e-6 per cell and scale, NMSE sums within 1e-10 relative (the
gates of tests/test_gpu_softmetrics.py).

Monotonicity (perfect-CSI LMMSE: BMI at 12 dB above BMI at 0 dB, no non-finite LLR) was first
confirmed for the numpy reference alone, on the CPU: tests/lmmse_ref.py on the slots of
oracle/synth_ref.py with this seed and these offsets gives BMI 0.4850 at 0 dB and 0.9777 at 12 dB,
nonfinite 0 (and for LS + nearest-neighbour estimates 0.2687 / 0.8375, with the GMI of the 12 dB
point at scale 0.707: 0.8515).
"""
import functools

import numpy as np
import pytest

from neural_rx_amd import softmetrics as SM
from tests import softmetrics_ref as R

pytestmark = pytest.mark.gpu

B, ITERS, EBNO = 8, 2, (0.0, 12.0)
SYSTEMS = ("nrx", "baseline_perf_csi_lmmse", "baseline_lsnn_lmmse")
KW = dict(max_mc_iter=ITERS, num_target_block_errors=10 ** 9, early_stop=False)


@functools.lru_cache(maxsize=None)
def _setup():
    from neural_rx_amd import weights as W
    from neural_rx_amd.config import get_config
    from neural_rx_amd.generator import GenParams, SlotGenerator
    from neural_rx_amd.receiver import CGNNEngine, spec_for
    cfg = get_config("nrx_rt")
    engine = CGNNEngine(spec_for(cfg), W.load(cfg.label))
    p = GenParams.from_config(cfg, num_prbs=4)
    return cfg, engine, p, SlotGenerator(p, want_h=True)


def _replay(system):
    """per Eb/N0 point: the reference sums of the receiver's own outputs on the loop's slots"""
    import torch
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.generator import ebno_to_no
    from neural_rx_amd.receiver import compute_pe
    cfg, engine, p, gen = _setup()
    pe = torch.from_numpy(compute_pe(p.num_tx, p.num_subcarriers, p.dmrs_symbols, p.cdm_group)).cuda()
    rx = None if system == "nrx" else BaselineReceiver(system, p)
    out = []
    for k, ebno in enumerate(EBNO):
        no = ebno_to_no(ebno, len(p.dmrs_symbols))
        tot = None
        for it in range(ITERS):
            sb = gen(B, no, slot_offset=(k * ITERS + it) * B)
            if rx is None:
                llr, h_est = engine.forward(sb.y, pe, sb.h_hat, sb.active, num_it=cfg.num_nrx_iter_eval, want_h=True)
            else:
                llr, h_est = rx(sb, no), rx.last_h
            torch.cuda.synchronize()
            host = lambda t: t.cpu().numpy()  # noqa: E731
            s = list(R.llr_stats(host(llr), host(sb.bits), host(sb.active), host(sb.mcs), p.mcs_bits, p.dmrs_symbols,
                                 SM.DEFAULT_SCALES))
            s += list(R.chest_nmse(host(h_est), host(sb.h), host(sb.active))) if h_est is not None else []
            tot = s if tot is None else [a + b for a, b in zip(tot, s)]
        out.append(tot)
    return out


@functools.lru_cache(maxsize=None)
def _sim(system, soft):
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.evaluate import sim_ber, sim_ber_baseline
    cfg, engine, p, gen = _setup()
    points = [] if soft else None
    if system == "nrx":
        res = sim_ber(engine, gen, EBNO, B, num_it=cfg.num_nrx_iter_eval, soft=points, **KW)
    else:
        res = sim_ber_baseline(BaselineReceiver(system, p), gen, EBNO, B, soft=points, **KW)
    return res, points


@pytest.mark.parametrize("system", SYSTEMS)
def test_counts_are_unchanged_by_soft(system):
    plain, none = _sim(system, False)
    res, points = _sim(system, True)
    assert none is None and len(points) == len(EBNO)
    assert res.counts == plain.counts and res.mc_iters == plain.mc_iters == [ITERS] * 2
    assert res.ber == plain.ber and res.bler == plain.bler and res.slots == plain.slots
    assert all(c[1] == ITERS * B * 2 * 48 * 12 * 4 for c in res.counts)


@pytest.mark.parametrize("system", SYSTEMS)
def test_soft_results_match_the_reference(system):
    _, p, _ = _setup()[1:]
    _, points = _sim(system, True)
    for ebno, sr, ref in zip(EBNO, points, _replay(system)):
        want = SM.derive(ref[0], ref[1], ref[2], p.mcs_bits, SM.DEFAULT_SCALES, *ref[3:])
        cells = np.asarray(want.cnt) > 0
        d = np.abs(np.asarray(sr.bmi_bits, float) - np.asarray(want.bmi_bits, float))[cells]
        print(f"{system} {ebno:5.1f} dB: BMI {sr.bmi[0]:.6f} (ref {want.bmi[0]:.6f})  GMI {sr.gmi[0]:.6f} "
              f"x{sr.gmi_scale[0]:g}  NMSE {sr.nmse}  max cell diff {d.max():.2e}")
        assert sr.cnt == want.cnt and sr.nonfinite == want.nonfinite == 0
        assert sum(map(sum, sr.cnt)) == ITERS * B * 2 * 48 * 12 * 4
        assert d.max() <= 1e-6
        assert abs(sr.bmi[0] - want.bmi[0]) <= 1e-6 and abs(sr.gmi[0] - want.gmi[0]) <= 1e-6
        # scale 1.0 is in the list, so the GMI is never below the BMI
        assert sr.gmi[0] >= sr.bmi[0]
        if system == "baseline_perf_csi_lmmse":
            assert sr.nmse is None and sr.nmse_user is None and want.nmse is None
        else:
            assert np.isfinite(sr.nmse) and sr.nmse > 0
            assert sr.channel_items == ITERS * B * 2
            assert abs(sr.nmse - want.nmse) <= 1e-10 * want.nmse
            np.testing.assert_allclose(sr.nmse_user, want.nmse_user, rtol=1e-10, atol=0)


def test_bmi_rises_with_ebno_for_perfect_csi():
    """the reference alone satisfies this on these slots (module docstring)"""
    _, points = _sim("baseline_perf_csi_lmmse", True)
    assert points[1].bmi[0] > points[0].bmi[0]
    assert points[0].nonfinite == 0 and points[1].nonfinite == 0
    assert 0.0 < points[0].bmi[0] < points[1].bmi[0] <= 1.0


def test_soft_needs_the_true_channel():
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.evaluate import sim_ber, sim_ber_baseline
    from neural_rx_amd.generator import SlotGenerator
    cfg, engine, p, _ = _setup()
    gen = SlotGenerator(p, want_h=False)
    with pytest.raises(ValueError, match="want_h=True"):
        sim_ber(engine, gen, EBNO, B, soft=[], **KW)
    with pytest.raises(ValueError, match="want_h=True"):
        sim_ber_baseline(BaselineReceiver("baseline_lsnn_lmmse", p), gen, EBNO, B, soft=[], **KW)
