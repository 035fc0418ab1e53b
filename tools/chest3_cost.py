"""Time the correlated-channel calls next to the calls they extend, with HIP events, all in one
process: nrx_chest_lmmse3 against nrx_chest_lmmse, nrx_generate_slots_ex (NULL chan, and a full chan
with per-port profiles and a mix) against nrx_generate_slots, nrx_cov_space_accumulate against
nrx_cov_accumulate.

    python tools/chest3_cost.py [--out FILE.json]

Shape: the bench shape (nrx_rt: 128 slots, 2 users, 4 PRB, 4 antennas).  Every figure is the median
over ROUNDS rounds of the mean over CALLS calls; within a round the calls of a pair alternate, so
clock and cache state drift hits both sides alike.  The spread (min .. max over the rounds) is
recorded beside every median.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, WARMUP, ROUNDS = 50, 5, 7


def _mean_us(call, calls=CALLS):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    from neural_rx_amd import _lib
    from neural_rx_amd.chest import ChannelEstimator, estimate_covariance
    from neural_rx_amd.config import get_config
    from neural_rx_amd.generator import GenParams, SlotGenerator, ebno_to_no, scenario
    lib = _lib.load()
    cfg = get_config("nrx_rt")
    plain = GenParams.from_config(cfg, num_prbs=4)
    corr = scenario("double_tdl_high", plain)
    B = 128
    no = ebno_to_no(5.0, len(plain.dmrs_symbols))
    gen_plain, gen_corr = SlotGenerator(plain, want_h=True), SlotGenerator(corr, want_h=True)
    cov = estimate_covariance(gen_corr, 256, 128)
    R_f, R_t = cov.matrices()
    sb = gen_corr(B, no)
    est2 = ChannelEstimator("lmmse", corr, R_f=R_f, R_t=R_t)
    est3 = ChannelEstimator("lmmse3", corr, R_f=R_f, R_t=R_t, R_s=cov.space())
    out2, out3 = torch.empty_like(sb.h), torch.empty_like(sb.h)

    # the generator through its three doors, writing the same buffers
    buf = gen_plain._alloc(B)
    d = plain.desc(B, no)
    o = _lib.nrx_gen_out()
    o.y, o.h_hat, o.h, o.active = (t.data_ptr() for t in (buf.y, buf.h_hat, buf.h, buf.active))
    o.mcs_mask, o.mcs, o.bits, o.bits_stride = buf.mcs_mask.data_ptr(), buf.mcs.data_ptr(), buf.bits.data_ptr(), plain.bits_max
    ws = torch.empty(gen_plain.workspace_bytes(B), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    full = gen_corr._chan

    def gen_old():
        _lib.check(lib.nrx_generate_slots(ctypes.byref(d), ctypes.byref(o), ws.data_ptr(), ws.numel(), st))

    def gen_null():
        _lib.check(lib.nrx_generate_slots_ex(ctypes.byref(d), None, ctypes.byref(o), ws.data_ptr(), ws.numel(), st))

    def gen_full():
        _lib.check(lib.nrx_generate_slots_ex(ctypes.byref(d), ctypes.byref(full), ctypes.byref(o), ws.data_ptr(),
                                             ws.numel(), st))

    # the two covariance calls on their own (CovarianceEstimator.accumulate makes both)
    lag = _lib.nrx_cov_io()
    spc = _lib.nrx_cov_space_io()
    for io in (lag, spc):
        io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = B, corr.num_tx, corr.num_subcarriers, 14
        io.num_rx_ant, io.h = corr.num_rx_ant, sb.h.data_ptr()
    acc_l = torch.zeros((corr.num_subcarriers + 14, 2), dtype=torch.float64, device="cuda")
    acc_s = torch.zeros((corr.num_rx_ant, corr.num_rx_ant, 2), dtype=torch.float64, device="cuda")
    lag.acc, spc.acc = acc_l.data_ptr(), acc_s.data_ptr()
    n = ctypes.c_size_t()
    _lib.check(lib.nrx_cov_workspace_size(ctypes.byref(lag), ctypes.byref(n)))
    ws_l = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    _lib.check(lib.nrx_cov_space_workspace_size(ctypes.byref(spc), ctypes.byref(n)))
    ws_s = torch.empty(n.value, dtype=torch.uint8, device="cuda")

    groups = {
        "chest": {"chest_lmmse": lambda: est2(sb, no, out=out2), "chest_lmmse3": lambda: est3(sb, no, out=out3)},
        "generate": {"generate_slots": gen_old, "generate_slots_ex_null": gen_null, "generate_slots_ex_full": gen_full},
        "cov": {"cov_accumulate": lambda: _lib.check(lib.nrx_cov_accumulate(ctypes.byref(lag), ws_l.data_ptr(),
                                                                            ws_l.numel(), st)),
                "cov_space_accumulate": lambda: _lib.check(lib.nrx_cov_space_accumulate(ctypes.byref(spc), ws_s.data_ptr(),
                                                                                        ws_s.numel(), st))},
    }
    r = dict(shape=dict(B=B, U=corr.num_tx, F=corr.num_subcarriers, A=corr.num_rx_ant), calls=CALLS, warmup=WARMUP,
             rounds=ROUNDS, build_id=lib.nrx_build_id().decode())
    for calls in groups.values():
        for call in calls.values():
            for _ in range(WARMUP):
                call()
        torch.cuda.synchronize()
        samples = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, call in calls.items():           # alternated: one timed run of each per round
                samples[k].append(_mean_us(call))
        for k, v in samples.items():
            r["us_" + k] = statistics.median(v)
            r["spread_" + k] = [min(v), max(v)]
    r["ratio_chest3_over_chest"] = r["us_chest_lmmse3"] / r["us_chest_lmmse"]
    r["ratio_ex_null_over_generate"] = r["us_generate_slots_ex_null"] / r["us_generate_slots"]
    r["ratio_ex_full_over_generate"] = r["us_generate_slots_ex_full"] / r["us_generate_slots"]
    r["ratio_cov_space_over_cov"] = r["us_cov_space_accumulate"] / r["us_cov_accumulate"]
    nm = lambda x: float(((x - sb.h) ** 2).sum() / (sb.h ** 2).sum())   # noqa: E731
    r["nmse_lmmse"], r["nmse_lmmse3"] = nm(out2), nm(out3)
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
