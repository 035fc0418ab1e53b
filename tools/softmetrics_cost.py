"""Time the soft-metric calls (nrx_llr_stats, nrx_chest_nmse) next to nrx_count_errors with HIP
events: the mean over 50 calls after 5 warm-ups, all in one process.

    python tools/softmetrics_cost.py [--out FILE.json]

Shape: the bench shape (nrx_rt: 128 slots, 2 users, 4 PRB, 4 antennas, 16-QAM).  The LLRs are the
LMMSE baseline's on generated slots at 6 dB, the channel estimate is the generator's h_hat.
nrx_llr_stats runs with one scale and with the nine default scales; nrx_count_errors, the kernel the
evaluation loop already runs on the same tensors, is the yardstick.  The forward of the same shape is
timed too, for the scale the DESIGN.md table quotes.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, WARMUP = 50, 5


def _mean_us(call):
    import torch
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3


def _kernel_us(calls: dict):
    """mean device time (us) per launch of every libnrx kernel the calls run, from the profiler (the
    event-timed figures include what the host needs to issue a call; these do not)"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for call in calls.values():
                for _ in range(CALLS):
                    call()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None)
            t = getattr(e, "cuda_time_total", 0.0) if t is None else t
            for tag in ("k_count_errors", "k_llr_partial", "k_llr_reduce", "k_nmse_partial", "k_nmse_reduce"):
                if tag in e.key and e.count:
                    out[tag] = dict(us=t / e.count, launches=e.count)
        return out or None
    except Exception as ex:  # optional: the event-timed figures do not depend on it
        print(f"profiler split unavailable: {ex}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    from neural_rx_amd import softmetrics as SM, weights as W
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.config import get_config
    from neural_rx_amd.generator import GenParams, SlotGenerator, count_errors, ebno_to_no
    from neural_rx_amd.receiver import CGNNEngine, compute_pe, spec_for
    cfg = get_config("nrx_rt")
    p = GenParams.from_config(cfg, num_prbs=4)
    B = 128
    no = ebno_to_no(6.0, len(p.dmrs_symbols))
    sb = SlotGenerator(p, want_h=True)(B, no)
    llr = BaselineReceiver("baseline_lsnn_lmmse", p)(sb, no)
    counts = torch.zeros((p.num_tx, 4), dtype=torch.int64, device="cuda")
    one, nine = SM.SoftAccumulator(p.num_tx, p.mcs_bits, (1.0,)), SM.SoftAccumulator(p.num_tx, p.mcs_bits)
    engine = CGNNEngine(spec_for(cfg), W.load(cfg.label))
    pe = torch.from_numpy(compute_pe(p.num_tx, p.num_subcarriers, p.dmrs_symbols, p.cdm_group)).cuda()
    out = engine.alloc_outputs(B, p.num_tx, p.num_subcarriers, want_h=True)
    r = dict(shape=dict(B=B, U=p.num_tx, F=p.num_subcarriers, A=p.num_rx_ant, bits_stride=p.bits_max), calls=CALLS,
             warmup=WARMUP)
    calls = {
        "count_errors": lambda: count_errors(llr, sb.bits, sb.active, sb.mcs, p.mcs_bits, p.dmrs_symbols, counts=counts),
        "llr_stats_s1": lambda: one.add_llr(llr, sb.bits, sb.active, sb.mcs, p.dmrs_symbols),
        "llr_stats_s9": lambda: nine.add_llr(llr, sb.bits, sb.active, sb.mcs, p.dmrs_symbols),
        "chest_nmse": lambda: nine.add_channel(sb.h_hat, sb.h, sb.active),
        "forward_f16": lambda: engine.forward(sb.y, pe, sb.h_hat, sb.active, num_it=cfg.num_nrx_iter_eval, out=out,
                                              want_h=True)}
    for name, call in calls.items():
        r["us_" + name] = _mean_us(call)
    # device time of the kernels alone (nrx_llr_stats with the nine scales)
    r["kernel_us"] = _kernel_us({k: v for k, v in calls.items() if k not in ("forward_f16", "llr_stats_s1")})
    res = nine.result()
    r["bmi"], r["gmi"], r["gmi_scale"], r["nmse"] = res.bmi, res.gmi, res.gmi_scale, res.nmse
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
