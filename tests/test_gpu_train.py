"""nrx_train_grad and nrx_adam_step on the GPU against the CPU oracle of tests/train_ref.py (needs an MI355X).

Gradient gate: per weight tensor the measure is ||g - g64|| / ||g64|| against the float64 autograd gradient; the
same oracle run in float32 gives e32, its worst tensor, and every tensor of the kernels must stay within
4 max(e32, 1e-6) -- the factor covers another, equally legitimate float32 summation order (k-ordered MFMA chains,
slab sums), nothing more.  The trajectory gate is the same rule on the total loss after every Adam step.
"""
import types

import numpy as np
import pytest
import torch

from tests import train_ref
from tests.memguard import Guarded, same_bits
from tests.test_gpu_parity import F32X_H_TOL, F32X_LLR_TOL
from tests.test_train_ref import TRAJ_STEPS, TRAJ_W_CHEST, trajectory_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def on_device(batch):
    """the oracle's batch as the tensors Trainer.grad takes (a generator.SlotBatch look-alike) and pe"""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    sb = types.SimpleNamespace(y=t(batch["y"]), h_hat=t(batch["h_hat"]), active=t(batch["active"]),
                               mcs_mask=t(batch["mcs_mask"]), bits=t(batch["bits"]), h=t(batch["h"]))
    return sb, t(batch["pe"])


def tensor_errors(grads, ref):
    """||g - ref|| / ||ref|| per array with a non-zero reference"""
    out = []
    for g, r in zip(grads, ref):
        r = np.asarray(r, np.float64)
        n = np.linalg.norm(r)
        if n > 0:
            out.append(float(np.linalg.norm(np.asarray(g, np.float64) - r) / n))
    return out


def check_gradient_parity(name, case, batch, sw, ref, ref32, guarded=False):
    """The gradient gate on one case: ``ref`` / ``ref32`` are ``train_ref.loss_and_grad`` in float64 (the truth)
    and float32 (the yardstick e32).  ``guarded``: the call runs in a NaN-filled ``memguard.Guarded`` workspace of
    exactly ``workspace_bytes(io)``, whose guard bands are checked.  Returns the figures and the gradients."""
    from neural_rx_amd.train import Trainer
    sp = case.spec
    sb, pe = on_device(batch)
    tr = Trainer(sp, case.weights)
    if guarded:
        io = tr._io(sb, pe, sw.get("num_it"), sw.get("multiloss", False), sw.get("w_chest", 0.0),
                    sw.get("dmrs_symbols", (2, 11)))
        ws = Guarded(tr.workspace_bytes(io), 0xFF)
        tr.g.fill_(float("nan"))
        tr.loss.fill_(float("nan"))
        llr, h_ref = tr.grad_async(sb, pe, want_outputs=True, workspace=ws.body, **sw)
    else:
        llr, h_ref = tr.grad_async(sb, pe, want_outputs=True, **sw)
    torch.cuda.synchronize()
    if guarded:
        ws.check(f"{name}: training workspace")
    grads, loss = tr.gradients(), tr.loss.tolist()

    e32 = max(tensor_errors(ref32["grads"], ref["grads"]))
    errs = tensor_errors(grads, ref["grads"])
    bound = 4 * max(e32, 1e-6)
    print(f"{name}: worst tensor {max(errs):.2e}  median {np.median(errs):.2e}  e32 {e32:.2e}  "
          f"ratio to the bound {max(errs) / bound:.3f}  loss {loss[0]:.6f} {loss[1]:.6f}")
    assert all(np.isfinite(g).all() for g in grads)
    assert max(errs) <= bound, (max(errs), bound, int(np.argmax(errs)))
    # dead units, inactive users, unused iterations: an exact zero stays an exact zero
    for i, (g, r) in enumerate(zip(grads, ref["grads"])):
        assert not g[r == 0].any(), i
    if "num_it" in sw:
        n_unused = sum(1 for r in ref["grads"] if not r.any())
        assert n_unused >= 13 * (sp.num_it - sw["num_it"])
    assert abs(loss[0] - ref["loss_data"]) <= 1e-6 * abs(ref["loss_data"])
    assert abs(loss[1] - ref["loss_chest"]) <= 1e-6 * abs(ref["loss_chest"])
    llr = llr.cpu().numpy()
    for m, nb in enumerate(sp.bits):
        head = llr[0 if sp.masking else m]
        assert np.abs(head[..., :nb] - ref["llr"][m]).max() < F32X_LLR_TOL
        if not sp.masking:
            assert not head[..., nb:].any()
    assert np.abs(h_ref.cpu().numpy() - ref["h_ref"]).max() < F32X_H_TOL
    return dict(e32=e32, worst=max(errs), ratio=max(errs) / bound, grads=grads, loss=loss)


@pytest.mark.parametrize("name", list(train_ref.CASES))
def test_gradient_parity(name):
    case, batch, sw = train_ref.build_case(name)
    ref = train_ref.loss_and_grad(case.weights, case.spec, **batch, **sw)
    ref32 = train_ref.loss_and_grad(case.weights, case.spec, **batch, **sw, dtype=torch.float32)
    check_gradient_parity(name, case, batch, sw, ref, ref32)


def test_no_channel_loss_without_h():
    """w_chest = 0 with h = NULL: loss_chest is 0 and the ChEst readout's arrays get no gradient"""
    from neural_rx_amd.train import Trainer
    case, batch, _ = train_ref.build_case("rt_b2_u2")
    batch = dict(batch, h=None)
    ref = train_ref.loss_and_grad(case.weights, case.spec, **batch)
    sb, pe = on_device(batch)
    tr = Trainer(case.spec, case.weights)
    ld, lc = tr.grad(sb, pe)
    grads = tr.gradients()
    assert lc == 0.0 and abs(ld - ref["loss_data"]) <= 1e-6 * ref["loss_data"]
    assert not any(g.any() for g in grads[-4:]) and all(g.any() for g in grads[-8:-4])


def test_reproducible_and_workspace_contract():
    """two calls give the same bits; so does a call in a NaN-filled workspace of exactly the size asked for, which
    leaves the guard bands around it alone"""
    from neural_rx_amd.train import Trainer
    case, batch, sw = train_ref.build_case("rt_multiloss")
    sb, pe = on_device(batch)
    tr = Trainer(case.spec, case.weights)
    runs = []
    for _ in range(2):
        tr.g.fill_(float("nan"))
        tr.grad_async(sb, pe, **sw)
        runs.append((tr.g.cpu().numpy(), tr.loss.cpu().numpy()))
    io = tr._io(sb, pe, None, sw["multiloss"], sw["w_chest"], (2, 11))
    for fill in (0xFF, 0x7B):
        ws = Guarded(tr.workspace_bytes(io), fill)
        tr.g.fill_(float("nan"))
        tr.grad_async(sb, pe, workspace=ws.body, **sw)
        runs.append((tr.g.cpu().numpy(), tr.loss.cpu().numpy()))
        ws.check("training workspace")
    for g, loss in runs[1:]:
        assert same_bits(g, runs[0][0]) and same_bits(loss, runs[0][1])
    assert np.isfinite(runs[0][0]).all()


def ulps(a, b):
    """distance in float32 steps (same-sign finite values)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def check_adam_step(n, step):
    """one nrx_adam_step on n elements against the numpy formula, within 2 ulp (w, m) and 4 ulp (v); from 96
    elements on, runs with g = 0, v = 0 and m = v = g = 0 are among them"""
    import ctypes
    from neural_rx_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(step)
    w = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
    m = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    v = (rng.uniform(0, 1, n) * 10.0 ** rng.uniform(-10, -2, n)).astype(np.float32)
    if n >= 96:
        g[:64] = 0.0                                  # no gradient: m and v only decay
        v[32:96] = 0.0                                # ... and where both are 0, eps alone is the denominator
        m[32:64] = 0.0
    want = train_ref.adam_step_f32(w, g, m, v, step)
    d = [torch.from_numpy(a.copy()).to(DEV) for a in (w, g, m, v)]
    io = _lib.nrx_adam_io()
    io.n, io.w, io.g, io.m, io.v = n, *(t.data_ptr() for t in d)
    io.lr, io.beta1, io.beta2, io.eps, io.step = 1e-3, 0.9, 0.999, 1e-7, step
    _lib.check(lib.nrx_adam_step(ctypes.byref(io), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got_w, got_g, got_m, got_v = (t.cpu().numpy() for t in d)
    assert same_bits(got_g, g)
    assert ulps(got_w, want[0]).max() <= 2 and ulps(got_m, want[1]).max() <= 2 and ulps(got_v, want[2]).max() <= 4
    # m and v against the plain float64 formula too (w reads the stored m and v, so it has no such twin)
    _, m64, v64 = train_ref.adam_step(*(a.astype(np.float64) for a in (w, g, m, v)), step)
    assert ulps(got_m, m64.astype(np.float32)).max() <= 2 and ulps(got_v, v64.astype(np.float32)).max() <= 4
    if n >= 96:
        assert same_bits(got_w[32:64], w[32:64])      # m = v = g = 0: w stays


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_step(step):
    check_adam_step(3 * 256 + 37, step)               # not a multiple of the workgroup


@pytest.fixture(scope="module")
def trained():
    """the fixed-batch Adam trajectory on the GPU: (trainer after the steps, batch on the device, pe, total loss
    before every step and after the last)"""
    from neural_rx_amd.train import Trainer
    case, batch = trajectory_case()
    sb, pe = on_device(batch)
    tr = Trainer(case.spec, case.weights)
    total = []
    for _ in range(TRAJ_STEPS):
        ld, lc = tr.grad(sb, pe, w_chest=TRAJ_W_CHEST)
        total.append(ld + TRAJ_W_CHEST * lc)
        tr.step()
    ld, lc = tr.grad(sb, pe, w_chest=TRAJ_W_CHEST)
    total.append(ld + TRAJ_W_CHEST * lc)
    return tr, case, batch, sb, pe, total


def test_adam_trajectory(trained):
    tr, case, batch, sb, pe, total = trained
    t64, _ = train_ref.trajectory(case.weights, case.spec, batch, TRAJ_STEPS, TRAJ_W_CHEST)
    t32, _ = train_ref.trajectory(case.weights, case.spec, batch, TRAJ_STEPS, TRAJ_W_CHEST, dtype=torch.float32)
    d_gpu = [abs(a - b) / b for a, b in zip(total, t64)]
    d_cpu = [abs(a - b) / b for a, b in zip(t32, t64)]
    print("total loss  gpu:", " ".join(f"{t:.7f}" for t in total))
    print("            f64:", " ".join(f"{t:.7f}" for t in t64))
    print("relative difference  gpu:", " ".join(f"{d:.1e}" for d in d_gpu), " cpu f32:", " ".join(f"{d:.1e}" for d in d_cpu))
    assert all(b < a for a, b in zip(total, total[1:])), total
    for k, (dg, dc) in enumerate(zip(d_gpu, d_cpu)):
        assert dg <= 4 * max(dc, 1e-6), (k, dg, dc)


def test_engine_takes_the_trained_weights(trained, tmp_path):
    """the hand-over keeps the Keras order: the engine's f32X LLRs on Trainer.weights() are the training forward's"""
    from neural_rx_amd import weights as W
    tr, case, batch, sb, pe, _ = trained
    llr, h_ref = tr.grad_async(sb, pe, w_chest=TRAJ_W_CHEST, want_outputs=True)
    eng = tr.engine()
    llr_e, h_e = eng.forward(sb.y, pe, sb.h_hat, sb.active, precision="f32x")
    torch.cuda.synchronize()
    assert (llr - llr_e).abs().max().item() < F32X_LLR_TOL and (h_ref - h_e).abs().max().item() < F32X_H_TOL
    # ... and they moved: the shipped-order check is not vacuous
    eng0 = type(eng)(case.spec, case.weights)
    llr_0, _ = eng0.forward(sb.y, pe, sb.h_hat, sb.active, precision="f32x")
    assert (llr - llr_0).abs().max().item() > 10 * F32X_LLR_TOL
    path = str(tmp_path / "trained.npz")
    W.save(path, tr.weights())
    assert all(same_bits(a, b) for a, b in zip(W.load_file(path), tr.weights()))
