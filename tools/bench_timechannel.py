"""Time of nrx_time_channel next to a device-to-device copy of the same input plus output bytes.

    python tools/bench_timechannel.py [--batch 128] [--users 2] [--antennas 4] [--paths 6] [--sinusoids 8]
                                      [--fft 4096] [--l_min -6] [--l_max 43] [--launches 200]

The operating point of DESIGN.md section 9: B = 128, U = 2, A = 4, L = 6, NS = 8, one slot at N = 4096 (Ls = 14 (N + cp)
= 61376 samples), 50 taps.  The kernel reads x once and writes r once, so a copy that moves the same bytes -- a
buffer of (x + r) / 2 bytes, read once and written once -- is the time an HBM-bound kernel could reach; the kernel
is bound by its f64 arithmetic instead (about 2 A U L NS rotations and U L span FIR terms per sample), and the
ratio says by how much.  Both are timed with HIP events around ``--launches`` back-to-back launches after a
warm-up, and one JSON line is printed.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, launches, warmup=10):
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
    ap.add_argument("--users", type=int, default=2)
    ap.add_argument("--antennas", type=int, default=4)
    ap.add_argument("--paths", type=int, default=6)
    ap.add_argument("--sinusoids", type=int, default=8)
    ap.add_argument("--fft", type=int, default=4096)
    ap.add_argument("--l_min", type=int, default=-6)
    ap.add_argument("--l_max", type=int, default=43)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args(argv)
    import torch
    from neural_rx_amd.ofdm import default_cp
    from neural_rx_amd.timechannel import TimeChannel
    B, U, A, L, NS, N = a.batch, a.users, a.antennas, a.paths, a.sinusoids, a.fft
    cp = default_cp(N)
    Ls, fs = 14 * (N + cp), N * 30e3
    f64 = dict(dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((B, U, Ls, 2), generator=g, **f64))
    g0 = torch.view_as_complex(torch.randn((B, U, A, L, NS, 2), generator=g, **f64))
    tau = torch.rand((B, U, L), generator=g, **f64) * ((a.l_max - 6) / fs)
    fd = (torch.rand((B, U, A, L, NS), generator=g, **f64) * 2 - 1) * 400.0
    chan = TimeChannel(fs, a.l_min, a.l_max, cp)
    r = chan(x, tau, g0, fd)
    nbytes = (x.numel() + r.numel()) * 16
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    t_chan = timed(lambda: chan(x, tau, g0, fd, out=r), a.launches)
    t_copy = timed(lambda: dst.copy_(src), a.launches)
    span = a.l_max - a.l_min + 1
    flops = B * Ls * (U * L * (A * NS * 8.0 + A * 8.0 + span * 4.0))        # rotate + add, g v, FIR (f64 flops)
    print(json.dumps(dict(batch=B, users=U, antennas=A, paths=L, sinusoids=NS, fft_size=N, num_samples=Ls, span=span,
                          launches=a.launches, bytes=nbytes, time_channel_us=round(t_chan, 1),
                          copy_us=round(t_copy, 1), time_channel_over_copy=round(t_chan / t_copy, 2),
                          time_channel_gbps=round(nbytes / t_chan * 1e-3, 1), copy_gbps=round(nbytes / t_copy * 1e-3, 1),
                          f64_tflops=round(flops / t_chan * 1e-6, 2))))


if __name__ == "__main__":
    main()
