"""Time the coded path of an evaluation batch (nrx_ldpc_gather, nrx_ldpc_decode, nrx_ldpc_count) next
to the forward and nrx_count_errors with HIP events: the mean over 50 calls after 5 warm-ups, all in
one process.

    python tools/ldpc_cost.py [--out FILE.json]

Shape: the bench shape (nrx_rt: 128 slots, 2 users, 4 PRB, 4 antennas, 16-QAM), so 256 codewords of
the r12 code at z = 96 (N = 2304).  The LLRs are the LMMSE baseline's on generated slots, at a low
Eb/N0 (most codewords run all 20 iterations), near the waterfall and above it (early stop after one
or two iterations); the decoder runs boxplus and min-sum, with and without early stop.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, WARMUP = 50, 5
EBNO = (0.0, 3.0, 8.0)


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    from neural_rx_amd import ldpc, weights as W
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.config import get_config
    from neural_rx_amd.generator import GenParams, SlotGenerator, count_errors, ebno_to_no
    from neural_rx_amd.receiver import CGNNEngine, compute_pe, spec_for
    cfg = get_config("nrx_rt")
    p = GenParams.from_config(cfg, num_prbs=4)
    B = 128
    gen = SlotGenerator(p, want_h=True)
    rx = BaselineReceiver("baseline_perf_csi_lmmse", p)
    code, C = ldpc.fit("r12", p.num_subcarriers * (14 - len(p.dmrs_symbols)) * max(p.mcs_bits))
    dec = ldpc.Decoder(code)
    engine = CGNNEngine(spec_for(cfg), W.load(cfg.label))
    pe = torch.from_numpy(compute_pe(p.num_tx, p.num_subcarriers, p.dmrs_symbols, p.cdm_group)).cuda()
    out = engine.alloc_outputs(B, p.num_tx, p.num_subcarriers)
    counts = torch.zeros((p.num_tx, 4), dtype=torch.int64, device="cuda")
    coded = torch.zeros((p.num_tx, 4), dtype=torch.int64, device="cuda")
    itc = torch.zeros((p.num_tx, 2), dtype=torch.int64, device="cuda")
    r = dict(shape=dict(B=B, U=p.num_tx, F=p.num_subcarriers, A=p.num_rx_ant, bits_stride=p.bits_max),
             code=dict(name="r12", mb=code.mb, nb=code.nb, z=code.z, n=code.n, cw_per_block=C,
                       codewords=B * p.num_tx * C, edges=int((code.shifts >= 0).sum()) * code.z),
             calls=CALLS, warmup=WARMUP, points=[])
    sb0 = gen(B, ebno_to_no(EBNO[0], len(p.dmrs_symbols)))
    r["us_forward_f16"] = _mean_us(lambda: engine.forward(sb0.y, pe, sb0.h_hat, sb0.active,
                                                          num_it=cfg.num_nrx_iter_eval, out=out))
    for ebno in EBNO:
        no = ebno_to_no(ebno, len(p.dmrs_symbols))
        sb = gen(B, no)
        llr = rx(sb, no)
        g = ldpc.gather(llr, sb.bits, sb.active, sb.mcs, p.mcs_bits, p.dmrs_symbols, C, code.n, code.n)
        pt = dict(ebno_db=ebno)
        pt["us_count_errors"] = _mean_us(
            lambda: count_errors(llr, sb.bits, sb.active, sb.mcs, p.mcs_bits, p.dmrs_symbols, counts=counts))
        pt["us_gather"] = _mean_us(
            lambda: ldpc.gather(llr, sb.bits, sb.active, sb.mcs, p.mcs_bits, p.dmrs_symbols, C, code.n, code.n, out=g))
        for cn in ("boxplus", "minsum"):
            for early in (True, False):
                o = dec.decode(g[0], 20, cn, early_stop=early, skip=g[1])
                key = f"us_decode_{cn}_{'early' if early else 'full'}"
                pt[key] = _mean_us(lambda: dec.decode(g[0], 20, cn, early_stop=early, skip=g[1], out=o))
                if early:
                    torch.cuda.synchronize()
                    pt[f"mean_iters_{cn}"] = float(o["iters"].float().mean())
                    pt[f"bler_{cn}"] = float((o["hard"][:, :code.num_info].any(dim=1)).float().mean())
        o = dec.decode(g[0], 20, "boxplus", early_stop=True, skip=g[1])
        pt["us_count"] = _mean_us(
            lambda: ldpc.count(o["hard"], g[1], B, p.num_tx, C, code.num_info, coded, o["iters"], itc))
        r["points"].append(pt)
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
