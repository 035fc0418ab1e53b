"""The NRX and the LMMSE baselines on more users than CDM groups, with and without cover-coded DMRS
ports, on the same slots (profiles/eval_cover_u4.json).

    python tools/cover_sweep.py [--users 4] [--dmrs_symbols 2 11] [--out profiles/eval_cover_u4.json]

Two arms per Eb/N0 point, same seed, same data bits: ``cover`` gives the users the ports of
``ls.DMRSPorts.for_config`` (h_hat is the despreading LS estimate), ``plain`` is the generator without
cover codes on the same CDM groups, where the users of a group collide on their pilots.  Systems: the
NRX (shipped weights, which saw ports 0 / 2 only), lsnn_lmmse, lmmse_lmmse (2-D filter, covariance from
2048 slots of its own arm) and perf_csi_lmmse.  More than 4 users need DMRS symbols in pairs
(``--dmrs_symbols 2 3 10 11``).
"""
import argparse
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="nrx_rt")
    ap.add_argument("--users", type=int, default=4)
    ap.add_argument("--prbs", type=int, default=4)
    ap.add_argument("--dmrs_symbols", type=int, nargs="+", default=None)
    ap.add_argument("--ebno_db", type=float, nargs="+", default=[4.0, 8.0, 12.0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=8, help="batches per Eb/N0 point")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from neural_rx_amd import _lib, chest
    from neural_rx_amd import weights as W
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.config import get_config
    from neural_rx_amd.evaluate import _sim_ber_nrx, sim_ber_baseline
    from neural_rx_amd.generator import GenParams, SlotGenerator
    from neural_rx_amd.ls import DMRSPorts
    from neural_rx_amd.receiver import CGNNEngine, spec_for
    assert torch.cuda.is_available(), "needs a HIP device"
    cfg = get_config(a.config)
    engine = CGNNEngine(spec_for(cfg), W.load(cfg.label))
    ports = DMRSPorts.for_config(cfg, a.users)
    base = GenParams.from_config(cfg, num_tx=a.users, num_prbs=a.prbs, seed=a.seed)
    if a.dmrs_symbols:
        base = dataclasses.replace(base, dmrs_symbols=tuple(a.dmrs_symbols))
    arms = {"cover": dataclasses.replace(base, dmrs=ports), "plain": dataclasses.replace(base, cdm_group=ports.cdm_group)}
    kw = dict(max_mc_iter=a.iters, num_target_block_errors=10**9, early_stop=False)
    out = dict(config=cfg.label, users=a.users, prbs=a.prbs, dmrs_symbols=list(base.dmrs_symbols), seed=a.seed,
               slots_per_point=a.batch * a.iters, ports=dataclasses.asdict(ports),
               build_id=_lib.load().nrx_build_id().decode(), arms={})
    for arm, p in arms.items():
        gen = SlotGenerator(p, want_h=True)
        res = {"nrx": _sim_ber_nrx(engine, gen, a.ebno_db, a.batch, a.iters, 10**9, None, False, cfg.num_nrx_iter_eval,
                                   "f16", True, 8, f"{arm} nrx")}
        cov = chest.estimate_covariance(gen, 2048, a.batch).matrices()
        for name in ("lsnn_lmmse", "lmmse_lmmse", "perf_csi_lmmse"):
            if name == "lmmse_lmmse" and p.dmrs is not None and p.dmrs.despread_t:
                continue        # out of scope: the estimators do not take time-despread pilots
            rx =chest.EstimatorBaselineReceiver("baseline_" + name, p, R_f=cov[0], R_t=cov[1]) \
                if name == "lmmse_lmmse" else BaselineReceiver("baseline_" + name, p)
            res[name] = sim_ber_baseline(rx, gen, a.ebno_db, a.batch, verbose=True, label=f"{arm} {name}", **kw)
        out["arms"][arm] = {k: dict(ebno_db=r.ebno_db, ber=r.ber, bler=r.bler, counts=r.counts) for k, r in res.items()}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
