"""K-best against LMMSE detection with perfect CSI where the gap is large: 4 users on 4 antennas.

    python tools/kbest_gap.py [--out FILE.json]

16-QAM, 4 PRB, ports on CDM groups (0, 1, 0, 1), 1 024 slots per point (8 batches of 128), the same
slots for both detectors (evaluate.sim_ber_baseline), uncoded BER.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--ebno_db", type=float, nargs="+", default=[6.0, 10.0, 14.0])
    ap.add_argument("--k", type=int, default=64)
    a = ap.parse_args()
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.evaluate import sim_ber_baseline
    from neural_rx_amd.generator import GenParams, SlotGenerator
    from neural_rx_amd.kbest import KBestBaselineReceiver
    p = GenParams(num_tx=4, num_subcarriers=48, num_rx_ant=4, cdm_group=(0, 1, 0, 1), mcs_bits=(4,), seed=1234)
    gen = SlotGenerator(p, want_h=True)
    kw = dict(batch_size=128, max_mc_iter=8, num_target_block_errors=10**9, early_stop=False, verbose=True)
    d = dict(num_tx=4, num_rx_ant=4, num_prbs=4, mcs_bits=[4], k=a.k, slots_per_point=1024)
    for name, rx in (("perf_csi_lmmse", BaselineReceiver("baseline_perf_csi_lmmse", p)),
                     ("perf_csi_kbest", KBestBaselineReceiver("baseline_perf_csi_kbest", p, k=a.k))):
        d[name] = sim_ber_baseline(rx, gen, a.ebno_db, label=name, **kw).as_dict()
    print(json.dumps(d))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(d, f)


if __name__ == "__main__":
    main()
