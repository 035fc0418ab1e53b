"""Time of one nrx_train_grad call (forward, loss and backward) and of one nrx_adam_step.

    python tools/bench_train.py [--config nrx_rt] [--prbs 4] [--batch 128] [--users 2] [--runs 20] [--multiloss]
                                [--micro_batch 32] [--num_gpus 8]

The bench configuration (nrx_rt, 4 PRB, B = 128, U = 2) on generated slots.  Every call is timed on its own with a
pair of HIP events after a warm-up; the JSON line gives the median, the extremes and the spread over ``--runs``
calls, the workspace, and the arithmetic: multiply-adds x 2 of the forward, of the backward-data products (every
layer but the first of each StateInit stack, whose input needs no gradient) and of the backward-weight products,
depthwise taps included, biases and elementwise work not -- and the rate that count gives at the median time.

``--micro_batch M`` times the step's gradient as micro-batches of M slots (``Trainer.grad_micro``: the first call
overwrites, the others accumulate) in the workspace of one micro-batch.  ``--num_gpus G`` starts G fresh processes,
one per GPU, each with its ``parallel.shard_range`` of the batch; ``grad_ms`` is then one rank's gradient calls plus
the all-reduce and ``allreduce_ms`` the all-reduce alone (rank 0's figures; the parent never touches a GPU).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def flops_per_position(spec, num_it, multiloss):
    """(forward, backward) multiply-adds x 2 per position"""
    sep = lambda ci, co: 9 * ci + ci * co            # noqa: E731
    stack = lambda ci: [sep(ci, 128), sep(128, 128), sep(128, spec.d_s)]        # noqa: E731
    init = stack(spec.init_in_ch)
    it = [spec.d_s * 64, 64 * spec.d_s] + stack(spec.update_in_ch)
    ro = sum(spec.d_s * 128 + 128 * b for b in spec.head_bits) + spec.d_s * 128 + 128 * 2 * spec.num_rx_ant
    nro = num_it if multiloss else 1
    fwd = spec.num_init * sum(init) + num_it * sum(it) + nro * ro
    bwd = 2 * fwd - spec.num_init * init[0]          # weight + data products, minus StateInit conv1's data product
    return 2.0 * fwd, 2.0 * bwd


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="nrx_rt")
    ap.add_argument("--prbs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--users", type=int, default=2)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--multiloss", action="store_true")
    ap.add_argument("--w_chest", type=float, default=0.02)
    ap.add_argument("--micro_batch", type=int, default=0, help="slots per gradient call (0: the whole batch)")
    ap.add_argument("--num_gpus", type=int, default=1, help="data-parallel ranks, one process per GPU (at most 16)")
    a = ap.parse_args(argv)
    if not 1 <= a.num_gpus <= 16 or a.micro_batch < 0:
        ap.error("--num_gpus must be 1..16 and --micro_batch >= 0")
    if a.num_gpus > 1:
        import multiprocessing as mp
        from neural_rx_amd.train import _free_port
        ctx, port = mp.get_context("spawn"), _free_port()
        procs = [ctx.Process(target=_rank, args=(r, a.num_gpus, port, a)) for r in range(a.num_gpus)]
        for p in procs:
            p.start()
        for p in procs:
            p.join()
        sys.exit(max(abs(p.exitcode or 0) for p in procs))
    bench(a)


def _rank(rank, world, port, a):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch
    import torch.distributed as dist
    torch.set_num_threads(max(1, int(os.environ.get("OMP_NUM_THREADS", "4")) // world))
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    try:
        bench(a, rank, world)
    finally:
        dist.destroy_process_group()


def bench(a, rank=0, world=1):
    import torch
    from neural_rx_amd import weights as W
    from neural_rx_amd.config import get_config
    from neural_rx_amd.generator import GenParams, SlotGenerator, ebno_to_no
    from neural_rx_amd.receiver import compute_pe, spec_for
    from neural_rx_amd.parallel import shard_range
    from neural_rx_amd.train import Trainer
    cfg = get_config(a.config)
    spec = spec_for(cfg)
    p = GenParams.from_config(cfg, num_tx=a.users, num_prbs=a.prbs)
    dev = torch.cuda.current_device()
    lo, hi = shard_range(a.batch, world, rank)
    sb = SlotGenerator(p, device=dev, want_h=True)(hi - lo, ebno_to_no(6.0, len(p.dmrs_symbols)), slot_offset=lo)
    pe = torch.from_numpy(compute_pe(p.num_tx, p.num_subcarriers, p.dmrs_symbols, p.cdm_group)).cuda()
    tr = Trainer(spec, W.load(cfg.label), device=dev)
    kw = dict(multiloss=a.multiloss, w_chest=a.w_chest, dmrs_symbols=p.dmrs_symbols)
    m = a.micro_batch or (hi - lo)
    # the micro-batches: views of the rank's slots (a slice along the slot axis is contiguous)
    micro = [type(sb)(**{k: (None if v is None else v[s:s + m]) for k, v in vars(sb).items()})
             for s in range(0, hi - lo, m)]

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return np.array(ms)

    def step_grad():
        if len(micro) == 1 and world == 1:
            tr.grad_async(sb, pe, **kw)
        else:
            tr.grad_micro(micro, pe, batch_total=a.batch, **kw)
        tr.all_reduce()

    g_ms = timed(step_grad)
    r_ms = timed(tr.all_reduce) if world > 1 else np.zeros(1)
    a_ms = timed(tr.step)
    if rank != 0:
        return
    P = (hi - lo) * a.users * p.num_subcarriers * 14
    fwd, bwd = flops_per_position(spec, spec.num_it, a.multiloss)
    med = float(np.median(g_ms))
    stat = lambda x: dict(median=round(float(np.median(x)), 4), min=round(float(x.min()), 4),     # noqa: E731
                          max=round(float(x.max()), 4), std=round(float(x.std()), 4))
    print(json.dumps(dict(config=cfg.label, batch=a.batch, users=a.users, prbs=a.prbs, positions=P, runs=a.runs,
                          multiloss=a.multiloss, w_chest=a.w_chest, micro_batch=m, calls=len(micro), num_gpus=world,
                          grad_ms=stat(g_ms), allreduce_ms=stat(r_ms), adam_ms=stat(a_ms),
                          num_weights=tr.w.numel(), workspace_bytes=int(tr._ws.buf.numel()),
                          gflop_forward=round(fwd * P * 1e-9, 2), gflop_backward=round(bwd * P * 1e-9, 2),
                          tflops=round((fwd + bwd) * P / med * 1e-9, 2), loss=tr.loss.tolist())))


if __name__ == "__main__":
    main()
