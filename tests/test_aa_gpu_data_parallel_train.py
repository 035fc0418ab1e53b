"""The data-parallel training step as product code: two ranks on one GPU (needs an MI355X).

Two processes share device 0 (gloo carries the gradient sum, since RCCL needs one device per rank) and each runs the
real ``train.train_loop``: per-slot Eb/N0, ``-micro_batch 1``, a global batch of 4 slots, so every rank accumulates
its two micro-batches with ``batch_total = 4`` and then all-reduces.  A third process runs the same steps alone, as
four micro-batches.  Every draw of a step is a function of (seed, step) and of global slot indices, so all three see
the same slots and the same Eb/N0; what differs is the float32 summation order of the gradient.

As in tests/test_aa_gpu_distributed.py the children are fresh interpreters, spawned when this module is set up.  This
file sorts before that one and before every other GPU test module, and its pytest process never initialises the
GPU: all GPU work -- the single-process comparison included -- happens in the children, which send numpy results
back over a queue.  The oracle (tests/train_ref.py) runs here, on the CPU.
"""
import os
import queue as queue_mod
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BG, STEPS, SEED = 4, 3, 5
# STEPS + 1 steps are run: the loss of step STEPS is the loss after the last of the STEPS Adam updates that count
ARGV = ["-config_name", "nrx_rt", "-num_prbs", "1", "-init", "seeded", "-seed", str(SEED), "-steps", str(STEPS + 1),
        "-batch_size", str(BG), "-micro_batch", "1", "-per_slot_ebno", "-ebno_db_min", "0", "-ebno_db_max", "10",
        "-eval_every", "1000000"]
W_CHEST, LR = 0.02, 1e-3            # the defaults of the command line
FIELDS = ("y", "h_hat", "active", "bits", "h")
WAIT = 300


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q):
    try:
        import torch
        from neural_rx_amd import train
        if world > 1:
            os.environ["MASTER_ADDR"] = "127.0.0.1"
            os.environ["MASTER_PORT"] = str(port)
            import torch.distributed as dist
            dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        a = train._arguments(ARGV)
        a.keep_batches = True
        out = dict(loss=[], slots=[], calls=[])

        def record(k, tr, kept):
            torch.cuda.synchronize()
            out["loss"].append(tr.loss.tolist())
            out["calls"].append(len(kept))
            out["slots"].append([{f: getattr(sb, f).cpu().numpy() for f in FIELDS} for sb in kept])
            if k == 0:
                out["g"] = tr.g.cpu().numpy()
                out["grads"] = tr.gradients()
            if k == STEPS:              # before the update of step STEPS: the state after STEPS updates
                out.update(w=tr.w.cpu().numpy(), m=tr.m.cpu().numpy(), v=tr.v.cpu().numpy(), num_steps=tr.num_steps)

        train.train_loop(a, rank, world, device=0, record=record, log=lambda *args, **kw: None)
        from neural_rx_amd.config import get_config
        from neural_rx_amd.generator import GenParams
        from neural_rx_amd.receiver import compute_pe
        p = GenParams.from_config(get_config("nrx_rt"), num_prbs=1)
        out["pe"] = compute_pe(p.num_tx, p.num_subcarriers, p.dmrs_symbols, p.cdm_group)
        q.put((rank, world, out, None))
        if world > 1:
            dist.destroy_process_group()
    except Exception as e:          # report instead of hanging the parent
        import traceback
        q.put((rank, world, None, repr(e) + "\n" + traceback.format_exc()))


def _collect(ctx, world):
    """start ``world`` ranks, wait for their results (every wait has a limit), {rank: (result, error)}"""
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in procs:
            try:
                rank, _, out, err = q.get(timeout=WAIT)
            except queue_mod.Empty:
                break
            got[rank] = (out, err)
            if err is not None:
                break
    finally:
        for p in procs:
            p.join(timeout=5 if len(got) < world or any(e for _, e in got.values()) else 60)
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    for r in range(world):
        got.setdefault(r, (None, f"rank {r} of {world} sent no result (exit code {procs[r].exitcode})"))
    return got


@pytest.fixture(scope="module")
def runs():
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    two = _collect(ctx, 2)
    errors = [e for _, e in two.values() if e is not None]
    if errors:
        return dict(errors=errors)
    one = _collect(ctx, 1)                 # only after both ranks have returned without error
    if one[0][1] is not None:
        return dict(errors=[one[0][1]])
    return dict(errors=[], r0=two[0][0], r1=two[1][0], single=one[0][0])


@pytest.fixture(scope="module")
def oracle(runs):
    """The CPU trajectories in float64 and float32 on the slots the single process generated: the total loss of
    every step, and step 0's gradients"""
    import torch
    from neural_rx_amd import weights as W
    from neural_rx_amd.config import get_config, spec_from_config
    from tests import train_ref
    assert not runs["errors"], runs["errors"]
    spec = spec_from_config(get_config("nrx_rt"))
    single = runs["single"]
    batches = []
    for pieces in single["slots"]:
        b = {f: np.concatenate([p[f] for p in pieces]) for f in FIELDS}
        batches.append(dict(b, pe=single["pe"], mcs_mask=None))
    res = {}
    for dtype, np_t in ((torch.float64, np.float64), (torch.float32, np.float32)):
        w = [np.asarray(a, np_t) for a in W.seeded(spec, SEED)]
        m, v = [np.zeros_like(a) for a in w], [np.zeros_like(a) for a in w]
        total, first = [], None
        for k, batch in enumerate(batches):
            r = train_ref.loss_and_grad(w, spec, w_chest=W_CHEST, dtype=dtype, **batch)
            first = first or r
            total.append(r["loss_data"] + W_CHEST * r["loss_chest"])
            if k == STEPS:
                break
            for i, g in enumerate(r["grads"]):
                w[i], m[i], v[i] = (x.astype(np_t) for x in train_ref.adam_step(w[i], g.astype(np_t), m[i], v[i], k + 1, lr=LR))
        res[np_t] = (total, first)
    return res[np.float64], res[np.float32], batches


def test_children_ran(runs):
    assert not runs["errors"], "\n".join(runs["errors"])
    assert runs["r0"]["calls"] == runs["r1"]["calls"] == [2] * (STEPS + 1)       # two micro-batches per rank and step
    assert runs["single"]["calls"] == [4] * (STEPS + 1)
    assert runs["r0"]["num_steps"] == runs["r1"]["num_steps"] == runs["single"]["num_steps"] == STEPS


def test_every_rank_sees_the_slots_of_their_global_index(runs):
    assert not runs["errors"], runs["errors"]
    for k in range(STEPS + 1):
        shard = runs["r0"]["slots"][k] + runs["r1"]["slots"][k]
        for b, (mine, theirs) in enumerate(zip(shard, runs["single"]["slots"][k])):
            for f in FIELDS:
                assert mine[f].tobytes() == theirs[f].tobytes(), (k, b, f)
    # the number of active users of step k is the loop's (seed, k) draw, the same in every slot of the step
    from neural_rx_amd import train
    for k, pieces in enumerate(runs["single"]["slots"]):
        active = np.concatenate([p["active"] for p in pieces])
        assert active.shape == (BG, 2) and (active.sum(axis=1) == train.sample_num_tx(SEED, k, 1, 2)).all(), k


def test_ranks_hold_the_same_bits(runs):
    assert not runs["errors"], runs["errors"]
    r0, r1 = runs["r0"], runs["r1"]
    assert r0["g"].tobytes() == r1["g"].tobytes() and np.isfinite(r0["g"]).all() and r0["g"].any()
    for name in ("w", "m", "v"):
        assert r0[name].tobytes() == r1[name].tobytes(), name
    assert r0["loss"] == r1["loss"]


def test_first_gradient_against_the_oracle(runs, oracle):
    from tests.test_train_ref import tensor_errors
    (t64, first64), (t32, first32), _ = oracle
    e32 = max(tensor_errors(first32["grads"], first64["grads"]))
    bound = 4 * max(e32, 1e-6)
    for name in ("r0", "single"):
        errs = tensor_errors(runs[name]["grads"], first64["grads"])
        print(f"{name}: worst tensor {max(errs):.2e}  e32 {e32:.2e}  ratio to the bound {max(errs) / bound:.3f}")
        assert max(errs) <= bound, (name, max(errs), bound)
        ld, lc = runs[name]["loss"][0]
        assert abs(ld - first64["loss_data"]) <= 1e-6 * first64["loss_data"]
        assert abs(lc - first64["loss_chest"]) <= 1e-6 * first64["loss_chest"]


def test_two_ranks_follow_the_single_process(runs, oracle):
    (t64, _), (t32, _), _ = oracle
    total = {n: [ld + W_CHEST * lc for ld, lc in runs[n]["loss"]] for n in ("r0", "single")}
    d32 = [abs(a - b) / b for a, b in zip(t32, t64)]
    print("total loss  two ranks:", " ".join(f"{t:.7f}" for t in total["r0"]))
    print("               single:", " ".join(f"{t:.7f}" for t in total["single"]))
    print("                  f64:", " ".join(f"{t:.7f}" for t in t64), " cpu f32 distance:", " ".join(f"{d:.1e}" for d in d32))
    assert len(t64) == len(total["r0"]) == len(total["single"]) == STEPS + 1
    for k in range(STEPS + 1):
        bound = 4 * max(d32[k], 1e-6)
        assert abs(total["r0"][k] - total["single"][k]) / t64[k] <= bound, (k, total["r0"][k], total["single"][k], bound)
