"""Time the despreading LS estimator (nrx_ls_estimate) with HIP events: median of 20 launches after 3
warm-ups, next to nrx_chest_lin -- the project's pure streaming kernel writing the same grid -- on the
same box and shape.

    python tools/ls_throughput.py [--out profiles/ls_throughput.json]

Shapes: the bench shape (nrx_rt: 128 slots, ports 0 / 2, 4 PRB, 4 antennas, DMRS symbols 2 11) and the
shard of BASELINE cfg5 (32 slots, 8 cover-coded ports, 273 PRB, 4 antennas, DMRS symbols 2 3 10 11).
Inputs are random (the kernels' time does not depend on the values).  Compulsory bytes of the
estimator: the nd DMRS rows of y in (B F nd 2A floats), the pilot table, and the grid out
(B U F 14 2A floats), plus the Aerial list (B nd F/2 U 2A floats) where it is asked for; the rate is
set against the 6.29 TB/s device copy rate.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29
SHAPES = {"bench": dict(B=128, ports=(0, 2), F=48, A=4, dmrs=(2, 11)),
          "cfg5_shard": dict(B=32, ports=tuple(range(8)), F=273 * 12, A=4, dmrs=(2, 3, 10, 11))}


def timed(call, launches=20, warmup=3):
    import torch
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
    return ms[len(ms) // 2], ms[0], ms[-1]


def run(name, B, ports, F, A, dmrs):
    import torch
    from neural_rx_amd.chest import ChannelEstimator
    from neural_rx_amd.generator import GenParams, SlotBatch
    from neural_rx_amd.ls import DMRSPorts, LSEstimator
    pt = DMRSPorts.from_ports(ports)
    U, nd = pt.num_tx, len(dmrs)
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.randn((B, F, 14, 2 * A), device="cuda", generator=g)
    pil = torch.sign(torch.randn((2, (F + 1) // 2, nd, 2), device="cuda", generator=g))
    act = torch.ones((B, U), device="cuda")
    b_out = B * U * F * 14 * 2 * A * 4
    b_in = B * F * nd * 2 * A * 4 + pil.numel() * 4
    rs = []
    for aerial in (False, True):
        est = LSEstimator(pt, F, A, dmrs, aerial=aerial)
        med, lo, hi = timed(lambda: est(y, pil, act))
        nbytes = b_in + b_out + (B * nd * (F // 2) * U * 2 * A * 4 if aerial else 0)
        out = est(y, pil, act)
        rs.append(dict(shape=name, kernel="nrx_ls_estimate" + (" + Aerial list" if aerial else ""), B=B, U=U, F=F, A=A,
                       dmrs_symbols=list(dmrs), despread=[int(pt.despread_f), int(pt.despread_t)], ms_median=med,
                       ms_min=lo, ms_max=hi, bytes_out=b_out, bytes_compulsory=nbytes, gbs=nbytes / med / 1e6,
                       fraction_of_copy_rate=nbytes / med / 1e9 / COPY_TBS,
                       finite=bool(torch.isfinite(out[0] if aerial else out).all())))
    # nrx_chest_lin on the same grid: reads the own pilots of a [B, U, F, 14, 2A] grid, writes one
    p = GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A, dmrs_symbols=dmrs, cdm_group=pt.cdm_group)
    hh = est(y, pil, act)[0]
    sb = SlotBatch(y=None, h_hat=hh, active=act, mcs_mask=None, mcs=None, bits=None)
    lin = ChannelEstimator("lin", p)
    out = torch.empty_like(hh)
    med, lo, hi = timed(lambda: lin(sb, 0.1, out=out))
    nbytes = B * U * (F // 2) * nd * 2 * A * 4 + b_out
    rs.append(dict(shape=name, kernel="nrx_chest_lin", B=B, U=U, F=F, A=A, dmrs_symbols=list(dmrs), ms_median=med,
                   ms_min=lo, ms_max=hi, bytes_out=b_out, bytes_compulsory=nbytes, gbs=nbytes / med / 1e6,
                   fraction_of_copy_rate=nbytes / med / 1e9 / COPY_TBS, finite=bool(torch.isfinite(out).all())))
    for r in rs:
        print(json.dumps(r), flush=True)
    return rs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from neural_rx_amd import _lib
    assert torch.cuda.is_available(), "needs a HIP device"
    rs = [r for n, s in SHAPES.items() for r in run(n, **s)]
    d = dict(device=torch.cuda.get_device_name(0), build_id=_lib.load().nrx_build_id().decode(),
             copy_rate_tbs=COPY_TBS, results=rs)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(d, f, indent=1)


if __name__ == "__main__":
    main()
