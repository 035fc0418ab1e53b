"""Time of nrx_ofdm_demodulate (and nrx_ofdm_modulate) next to a device-to-device copy of the same bytes.

    python tools/bench_ofdm.py [--batch 128] [--streams 4] [--fft 4096] [--subcarriers 1584] [--launches 200]

The demodulator reads every sample once and writes every grid element once, so a copy that moves the same
bytes -- a buffer of (samples + grid) / 2 bytes, read once and written once -- on the same machine is the time an
HBM-bound kernel could reach.  Both are timed with HIP events around
``--launches`` back-to-back launches after a warm-up, and one JSON line is printed.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, launches, warmup=20):
    import torch
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches          # us per launch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--fft", type=int, default=4096)
    ap.add_argument("--subcarriers", type=int, default=1584)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--precision", default="f32", choices=["f32", "f64"])
    ap.add_argument("--layout", default="cgnn", choices=["cgnn", "planar"])
    a = ap.parse_args(argv)
    import torch
    from neural_rx_amd.ofdm import OFDMDemodulator, OFDMModulator, default_cp
    B, S, N, F = a.batch, a.streams, a.fft, a.subcarriers
    cp = default_cp(N)
    cdt = torch.complex64 if a.precision == "f32" else torch.complex128
    L = 14 * (N + cp)
    smp = torch.view_as_complex(torch.randn((B, S, L, 2), dtype=cdt.to_real(), device="cuda"))
    demod = OFDMDemodulator(N, 0, cp, num_subcarriers=F, layout=a.layout, precision=a.precision)
    mod = OFDMModulator(cp, fft_size=N, layout=a.layout, precision=a.precision)
    grid = demod(smp)
    out_s = torch.empty_like(smp)
    nbytes = smp.numel() * smp.element_size() + grid.numel() * grid.element_size()
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    t_demod = timed(lambda: demod(smp, out=grid), a.launches)
    t_mod = timed(lambda: mod(grid, out=out_s), a.launches)
    t_copy = timed(lambda: dst.copy_(src), a.launches)
    print(json.dumps(dict(batch=B, streams=S, fft_size=N, subcarriers=F, cp=cp, precision=a.precision, layout=a.layout,
                          launches=a.launches, bytes=nbytes, demodulate_us=round(t_demod, 2),
                          modulate_us=round(t_mod, 2), copy_us=round(t_copy, 2),
                          demodulate_over_copy=round(t_demod / t_copy, 3),
                          demodulate_gbps=round(nbytes / t_demod * 1e-3, 1), copy_gbps=round(nbytes / t_copy * 1e-3, 1))))


if __name__ == "__main__":
    main()
