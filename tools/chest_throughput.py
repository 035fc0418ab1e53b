"""Time the channel-estimation kernels (nrx_chest_lmmse, nrx_chest_lin) with HIP events: 20 launches
after 3 warm-ups.

    python tools/chest_throughput.py [--out profiles/chest_throughput.json]

Shapes: the bench shape (nrx_rt: 128 slots, 2 users, 4 PRB, 4 antennas) and BASELINE cfg3's
(64 slots, 4 users, 132 PRB, 16 antennas), DMRS symbols (2, 11).  Inputs are random (the kernels'
time does not depend on the values) and the filter comes from chest.lmmse_design on an analytic
covariance.  Compulsory bytes: the own pilots in (B U |P| nd 2A floats), the filter table once
(lmmse: both groups, nd F Pmax complex) and the grid out (B U F 14 2A floats); the rate is set
against the 6.29 TB/s device copy rate.  FLOPs of the LMMSE products: 8 F |P| nd A per (b, u).
"""
import argparse
import json
import os
import socket
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29
SHAPES = {"bench": dict(B=128, U=2, F=48, A=4), "cfg3": dict(B=64, U=4, F=132 * 12, A=16)}


def model_covariance(F, max_delay_s=300e-9, scs=30e3, max_doppler_hz=400.0, n=64):
    """exponential power-delay profile, uniform Doppler angles: positive semi-definite Toeplitz"""
    from neural_rx_amd.chest import toeplitz
    tau = (np.arange(n) + 0.5) / n * max_delay_s
    w = np.exp(-tau / (max_delay_s / 3.0))
    w /= w.sum()
    d = np.arange(F)[:, None]
    r_f = (w * np.exp(-2j * np.pi * d * scs * tau)).sum(-1)
    fd = max_doppler_hz * np.cos(2 * np.pi * (np.arange(n) + 0.5) / n)
    r_t = np.exp(2j * np.pi * fd * np.arange(14)[:, None] * (1.0 + 9.0 / 128.0) / scs).mean(-1)
    return toeplitz(r_f), toeplitz(r_t)


def run(name, kind, B, U, F, A, launches=20, warmup=3):
    import torch
    from neural_rx_amd.chest import ChannelEstimator, lmmse_design
    from neural_rx_amd.generator import GenParams, SlotBatch
    dmrs = (2, 11)
    p = GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A, dmrs_symbols=dmrs,
                  cdm_group=tuple(u % 2 for u in range(U)))
    g = torch.Generator(device="cuda").manual_seed(1)
    sb = SlotBatch(y=None, h_hat=torch.randn((B, U, F, 14, 2 * A), device="cuda", generator=g),
                   active=torch.ones((B, U), device="cuda"), mcs_mask=None, mcs=None, bits=None)
    tables = lmmse_design(*model_covariance(F), p, 0.1) if kind == "lmmse" else None
    est = ChannelEstimator(kind, p, tables=tables)
    out = torch.empty_like(sb.h_hat)
    call = lambda: est(sb, 0.1, out=out)  # noqa: E731
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
    med = ms[len(ms) // 2]
    npil = sum(len(range(p.cdm_group[u], F, 2)) for u in range(U))
    b_pil = B * npil * len(dmrs) * 2 * A * 4
    b_tab = tables.filt.nbytes if tables is not None else 0
    b_out = B * U * F * 14 * 2 * A * 4
    nbytes = b_pil + b_tab + b_out
    flops = 8.0 * F * B * npil * len(dmrs) * A if kind == "lmmse" else 0.0
    r = dict(shape=name, kernel="nrx_chest_" + kind, B=B, U=U, F=F, A=A, dmrs_symbols=list(dmrs), launches=launches,
             ms_median=med, ms_min=ms[0], ms_max=ms[-1], bytes_pilots=b_pil, bytes_table=b_tab, bytes_out=b_out,
             bytes_compulsory=nbytes, gbs=nbytes / med / 1e6, fraction_of_copy_rate=nbytes / med / 1e9 / COPY_TBS,
             tflops=flops / med / 1e9, finite=bool(torch.isfinite(out).all()))
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from neural_rx_amd import _lib
    assert torch.cuda.is_available(), "needs a HIP device"
    rs = [run(n, k, **s) for n, s in SHAPES.items() for k in ("lmmse", "lin")]
    d = dict(box=socket.gethostname(), device=torch.cuda.get_device_name(0),
             build_id=_lib.load().nrx_build_id().decode(), copy_rate_tbs=COPY_TBS, results=rs)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(d, f, indent=1)


if __name__ == "__main__":
    main()
