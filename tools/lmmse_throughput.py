"""Time the LMMSE baseline kernel (nrx_lmmse_detect) with HIP events: 20 launches after 3 warm-ups.

    python tools/lmmse_throughput.py [--out FILE.json]

Shapes: the shard of BASELINE cfg5 (8 users, 273 PRB, 4 antennas, 32 slots, 64-QAM) and the bench
shape (nrx_rt: 2 users, 4 PRB, 4 antennas, 128 slots, 16-QAM).  Inputs are random (the kernel's
time does not depend on the values; |h| ~ 1 keeps every RE on the regular path).  Bytes per RE by
the algorithm: 8 A (U + 1) read + 4 U bits_stride written; the kernel skips the loads of the two
DMRS symbols, so the bytes it actually moves are reported next to that figure.  The rate is set
against the 6.29 TB/s device copy rate.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29
SHAPES = {"cfg5_shard": dict(B=32, U=8, F=273 * 12, A=4, bits=6), "bench": dict(B=128, U=2, F=48, A=4, bits=4)}


def run(name, B, U, F, A, bits, launches=20, warmup=3):
    import torch
    from neural_rx_amd.baseline import LMMSEDetector
    T, dmrs = 14, (2, 11)
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.randn((B, F, T, 2 * A), device="cuda", generator=g)
    h = torch.randn((B, U, F, T, 2 * A), device="cuda", generator=g)
    active = torch.ones((B, U), device="cuda")
    out = torch.empty((1, B, U, F, T, bits), device="cuda")
    det = LMMSEDetector()
    call = lambda: det(y, h, active, None, (bits,), 0.1, dmrs, out=out)  # noqa: E731
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
    ev[0].record()
    for i in range(launches):
        call()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(launches))
    res = B * F * T
    nominal = res * (8 * A * (U + 1) + 4 * U * bits)
    moved = res * (T - len(dmrs)) // T * 8 * A * (U + 1) + res * 4 * U * bits
    med = ms[len(ms) // 2]
    r = dict(shape=name, B=B, U=U, F=F, A=A, bits_stride=bits, resource_elements=res, launches=launches,
             ms_median=med, ms_min=ms[0], ms_max=ms[-1], bytes_nominal=nominal, bytes_moved=moved,
             tbs_nominal=nominal / med / 1e9, tbs_moved=moved / med / 1e9,
             fraction_of_copy_rate=moved / med / 1e9 / COPY_TBS, finite=bool(torch.isfinite(out).all()))
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    rs = [run(n, **s) for n, s in SHAPES.items()]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rs, f, indent=1)


if __name__ == "__main__":
    main()
