"""Time the channel-impulse-response replay (nrx_generate_slots_cir) with HIP events: median of 20 calls after 3
warm-ups.

    python tools/cir_throughput.py [--out profiles/cir_throughput.json] [--parent-lib PATH/libnrx.so]

1. The bench shape (128 slots, 2 users, 4 PRB, 4 antennas): the replay of the exported taps of the same slots (6 paths,
   14 time steps) against the built-in nrx_generate_slots.  With --parent-lib the built-in side is also timed in a
   library built from the parent commit; the libraries alternate three times, each measurement in a fresh process.
2. The reference's evaluation shape (20 slots, 2 users, 132 PRB, 4 antennas) with 32 and 128 paths, 14 and 1 time steps,
   with and without normalisation, and with one path: the calls' other launches (parameters, transmit grid, noise, LS).
   The f64 rate counts 8 real FLOPs per complex multiply-add over B U A F 14 L and is set against the time of the call
   minus the one-path call -- the CIR to H product alone.

A call is a whole generator call: every launch of it is inside the events.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def built_in(lib_path, B=128, U=2, F=48, A=4):
    """nrx_generate_slots of the library at lib_path (any libnrx.so with that entry point), through plain ctypes"""
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.generator import GenParams
    lib = ctypes.CDLL(lib_path)
    p = GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A)
    d = p.desc(B, 0.05)
    n = ctypes.c_size_t()
    assert lib.nrx_gen_workspace_size(ctypes.byref(d), ctypes.byref(n)) == 0
    f32 = dict(dtype=torch.float32, device="cuda")
    y, h = torch.empty((B, F, 14, 2 * A), **f32), torch.empty((B, U, F, 14, 2 * A), **f32)
    hh, act, mask = torch.empty_like(h), torch.empty((B, U), **f32), torch.empty((B, U, 1), **f32)
    mcs = torch.empty((B, U), dtype=torch.uint8, device="cuda")
    bits = torch.empty((B, U, F, 14, 4), dtype=torch.uint8, device="cuda")
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    o = _lib.nrx_gen_out()
    o.y, o.h_hat, o.h, o.active, o.mcs_mask, o.mcs = (t.data_ptr() for t in (y, hh, h, act, mask, mcs))
    o.bits, o.bits_stride = bits.data_ptr(), 4
    lib.nrx_generate_slots.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    st = torch.cuda.current_stream().cuda_stream

    def call():
        assert lib.nrx_generate_slots(ctypes.byref(d), ctypes.byref(o), ws.data_ptr(), ws.numel(), st) == 0
    med, lo, hi = timed(call)
    lib.nrx_build_id.restype = ctypes.c_char_p
    return dict(what="nrx_generate_slots", lib=os.path.basename(lib_path), build_id=lib.nrx_build_id().decode(), B=B, U=U, F=F, A=A,
                ms_median=med, ms_min=lo, ms_max=hi, finite=bool(torch.isfinite(y).all()))


def replay_bench(B=128, U=2, F=48, A=4):
    import torch
    from neural_rx_amd.cir import CIRChannel
    from neural_rx_amd.generator import GenParams, SlotGenerator
    p = GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A)
    base = SlotGenerator(p, want_h=True)
    ds = base.export_taps(B)
    idx = torch.arange(B * U, dtype=torch.int32, device="cuda").reshape(B, U)
    import dataclasses
    gen = SlotGenerator(dataclasses.replace(p, cir=CIRChannel(ds, "index", False, "zero")), want_h=True)
    sb = gen(B, 0.05, cir_index=idx)
    med, lo, hi = timed(lambda: gen(B, 0.05, cir_index=idx))
    ref = base(B, 0.05)
    err = float((sb.h - ref.h).abs().max())
    return dict(what="nrx_generate_slots_cir (exported taps, L 6, Ta 14)", B=B, U=U, F=F, A=A, ms_median=med, ms_min=lo,
                ms_max=hi, max_abs_h_difference_to_built_in=err)


def replay_eval(L, Ta, normalize, B=20, U=2, F=132 * 12, A=4):
    import numpy as np
    import torch
    from neural_rx_amd.cir import CIRChannel, CIRDataset
    from neural_rx_amd.generator import GenParams, SlotGenerator
    rng = np.random.default_rng(L + Ta)
    E = 64
    a = (rng.standard_normal((E, A, L, Ta)) + 1j * rng.standard_normal((E, A, L, Ta))).astype(np.complex64)
    tau = np.sort(rng.uniform(0, 1e-6, (E, L)), -1).astype(np.float32)
    p = GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A, cir=CIRChannel(CIRDataset(a, tau), "trajectory", normalize))
    gen = SlotGenerator(p, want_h=True)
    sb = gen(B, 0.05)
    med, lo, hi = timed(lambda: gen(B, 0.05))
    return dict(what="nrx_generate_slots_cir", B=B, U=U, F=F, A=A, L=L, Ta=Ta, normalize=bool(normalize), ms_median=med,
                ms_min=lo, ms_max=hi, flop=8.0 * B * U * A * F * 14 * L, finite=bool(torch.isfinite(sb.y).all()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="a libnrx.so built from the parent commit")
    ap.add_argument("--one", default=None, help="internal: one measurement in this process, printed as JSON")
    a = ap.parse_args()
    import torch
    from neural_rx_amd import _lib
    assert torch.cuda.is_available(), "needs a HIP device"
    if a.one:
        r = built_in(a.one) if a.one != "replay" else replay_bench()
        print("RESULT " + json.dumps(r), flush=True)
        return
    rs = []

    def child(arg):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", arg], check=True, capture_output=True,
                             text=True, timeout=300).stdout
        r = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps(r), flush=True)
        rs.append(r)

    for _ in range(3):
        if a.parent_lib:
            child(os.path.abspath(a.parent_lib))
        child(_lib.LIB_PATH)
        child("replay")
    one_path = {}
    for normalize in (False, True):
        r = replay_eval(1, 1, normalize)
        one_path[normalize] = r["ms_median"]
        print(json.dumps(r), flush=True)
        rs.append(r)
    for L in (32, 128):
        for Ta in (14, 1):
            for normalize in (False, True):
                r = replay_eval(L, Ta, normalize)
                r["ms_minus_one_path"] = r["ms_median"] - one_path[normalize]
                r["tflops_f64_of_the_product"] = r["flop"] / (r["ms_minus_one_path"] * 1e-3) / 1e12
                r["tflops_f64_of_the_call"] = r["flop"] / (r["ms_median"] * 1e-3) / 1e12
                print(json.dumps(r), flush=True)
                rs.append(r)
    d = dict(device=torch.cuda.get_device_name(0), build_id=_lib.load().nrx_build_id().decode(), results=rs)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(d, f, indent=1)


if __name__ == "__main__":
    main()
