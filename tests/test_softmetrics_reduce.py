"""SoftAccumulator.reduce over two gloo ranks (CPU): each rank holds host accumulators filled from
the numpy reference on its half of a batch; after the reduction both hold the sums of the whole."""
import os
import socket

import numpy as np
import torch.multiprocessing as mp

from tests import softmetrics_ref as R

MCS_BITS, DMRS, SCALES = (2, 4), (2, 11), (0.5, 1.0, 2.0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _batch():
    rng = np.random.default_rng(11)
    B, U, F, bs = 4, 3, 5, 4
    llr = (rng.standard_normal((2, B, U, F, 14, bs)) * 8).astype(np.float32)
    llr[0, 1, 0, 2, 5, 0] = np.nan
    bits = rng.integers(0, 2, (B, U, F, 14, bs)).astype(np.uint8)
    active = (rng.random((B, U)) < 0.8).astype(np.float32)
    mcs = rng.integers(0, 2, (B, U)).astype(np.uint8)
    h = rng.standard_normal((B, U, F, 14, 4)).astype(np.float32)
    he = (h + 0.1 * rng.standard_normal(h.shape)).astype(np.float32)
    return llr, bits, active, mcs, he, h


def _sums(lo, hi):
    llr, bits, active, mcs, he, h = _batch()
    loss, cnt, nonf = R.llr_stats(llr[:, lo:hi], bits[lo:hi], active[lo:hi], mcs[lo:hi], MCS_BITS, DMRS, SCALES)
    err, ref, items = R.chest_nmse(he[lo:hi], h[lo:hi], active[lo:hi])
    return dict(loss=loss, cnt=cnt, nonfinite=nonf, err=err, ref=ref, items=items)


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from neural_rx_amd.softmetrics import SoftAccumulator
    acc = SoftAccumulator(3, MCS_BITS, SCALES, device=None)
    for name, a in _sums(2 * rank, 2 * rank + 2).items():
        getattr(acc, name).copy_(torch.from_numpy(a))
    local = {k: v.copy() for k, v in acc.arrays().items()}
    acc.reduce(dist)
    tot = acc.arrays()
    res = acc.result()
    # the rank's own accumulators are left as they were
    kept = all(np.array_equal(getattr(acc, k).numpy(), local[k]) for k in local)
    q.put((rank, {k: v.tolist() for k, v in tot.items()}, res.as_dict(), kept))
    dist.destroy_process_group()


def test_gloo_two_ranks_hold_the_whole_batch():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res = {r: (tot, d, kept) for r, tot, d, kept in got}
    assert res[0][2] and res[1][2]
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    whole = _sums(0, 4)
    tot = res[0][0]
    for k in ("cnt", "nonfinite", "items"):
        assert np.array_equal(np.asarray(tot[k], np.int64), whole[k]), k
    assert whole["nonfinite"].sum() >= 0 and np.asarray(tot["cnt"]).sum() > 0
    for k in ("loss", "err", "ref"):
        np.testing.assert_allclose(np.asarray(tot[k]), whole[k], rtol=1e-12, atol=0, err_msg=k)
    from neural_rx_amd import softmetrics as SM
    ref = SM.derive(whole["loss"], whole["cnt"], whole["nonfinite"], MCS_BITS, SCALES, whole["err"], whole["ref"],
                    whole["items"])
    np.testing.assert_allclose(res[0][1]["bmi"], ref.bmi, rtol=0, atol=1e-12)
    assert abs(res[0][1]["nmse"] - ref.nmse) <= 1e-12 * ref.nmse
