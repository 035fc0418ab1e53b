"""Time the K-best detector (nrx_kbest_detect) with HIP events: 20 launches after 3 warm-ups.

    python tools/kbest_throughput.py [--out FILE.json]

Shapes: the bench shape (nrx_rt: 2 users, 4 PRB, 4 antennas, 128 slots, 16-QAM) and the shard of
BASELINE cfg3 (4 users, 132 PRB, 16 antennas, 64 slots, 16-QAM), k = 64.  Inputs are random
(|h| ~ 1: every RE is on the regular path; the control flow of the search depends on n, L and k
only, not on the values).  Every shape runs in a child process of its own under a time limit, and
the run stops at the first one that fails.  Per shape: the median time of the call (both kernels),
data REs per second, the pre-pass / search split from the profiler's kernel times of the same
launches (null if the profiler reports none), and nrx_lmmse_detect on the same tensors for scale.
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"bench": dict(B=128, U=2, F=48, A=4, bits=4), "cfg3_shard": dict(B=64, U=4, F=132 * 12, A=16, bits=4)}
STEP_TIMEOUT_S = 120


def _median_ms(call, launches, warmup):
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


def _kernel_split(call, launches):
    """mean device time (ms) of the two kernels over `launches` calls, from the profiler"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(launches):
                call()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None)
            t = getattr(e, "cuda_time_total", 0.0) if t is None else t
            for tag in ("k_kbest_gram", "k_kbest_search"):
                if tag in e.key and e.count:
                    out[tag] = out.get(tag, 0.0) + t / 1e3 / launches
        return out if len(out) == 2 else None
    except Exception as ex:  # the split is optional: the timed figures above do not depend on it
        print(f"profiler split unavailable: {ex}", file=sys.stderr)
        return None


def run(name, B, U, F, A, bits, k=64, launches=20, warmup=3):
    import torch
    from neural_rx_amd.baseline import LMMSEDetector
    from neural_rx_amd.kbest import KBestDetector
    T, dmrs = 14, (2, 11)
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.randn((B, F, T, 2 * A), device="cuda", generator=g)
    h = torch.randn((B, U, F, T, 2 * A), device="cuda", generator=g)
    active = torch.ones((B, U), device="cuda")
    out = torch.empty((1, B, U, F, T, bits), device="cuda")
    kb, lm = KBestDetector(), LMMSEDetector()
    call = lambda: kb(y, h, active, None, (bits,), 0.1, dmrs, k=k, out=out)  # noqa: E731
    med, lo, hi = _median_ms(call, launches, warmup)
    finite = bool(torch.isfinite(out).all())
    split = _kernel_split(call, launches)
    lmed, _, _ = _median_ms(lambda: lm(y, h, active, None, (bits,), 0.1, dmrs, out=out), launches, warmup)
    data_res = B * F * (T - len(dmrs))
    r = dict(shape=name, B=B, U=U, F=F, A=A, bits_stride=bits, k=k, data_resource_elements=data_res,
             launches=launches, ms_median=med, ms_min=lo, ms_max=hi, data_res_per_s=data_res / med * 1e3,
             ms_prepass=split and split["k_kbest_gram"], ms_search=split and split["k_kbest_search"],
             ms_lmmse_detect=lmed, times_lmmse=med / lmed, finite=finite)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, choices=list(SHAPES), help="run one shape in this process")
    a = ap.parse_args()
    if a.shape:
        import torch
        assert torch.cuda.is_available(), "needs a HIP device"
        run(a.shape, **SHAPES[a.shape])
        return
    rs = []
    for name in SHAPES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name], capture_output=True,
                           text=True, timeout=STEP_TIMEOUT_S)
        sys.stderr.write(p.stderr)
        if p.returncode:
            raise SystemExit(f"{name}: exit status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        rs.append(json.loads(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rs, f, indent=1)


if __name__ == "__main__":
    main()
