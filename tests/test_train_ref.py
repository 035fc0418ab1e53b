"""The training oracle (tests/train_ref.py) on its own, on the CPU: its forward against the numpy oracle, its
gradient against central finite differences, the loss normalisation by hand, and the Adam trajectory that
tests/test_gpu_train.py compares the kernels with."""
import numpy as np
import pytest
import torch

from oracle import cgnn_ref
from tests import train_ref
from tests.helpers import make_case

TRAJ_STEPS, TRAJ_W_CHEST = 6, 0.02


def trajectory_case():
    """seeded weights, nrx_rt topology, one fixed batch (B = 2, U = 2, 1 PRB)"""
    case = make_case("nrx_rt", batch=2, users=2, prbs=1, seeded_weights=True)
    return case, train_ref.training_batch(case)


@pytest.mark.parametrize("name", list(train_ref.CASES))
def test_forward_equals_the_numpy_oracle(name):
    case, batch, sw = train_ref.build_case(name)
    got = train_ref.loss_and_grad(case.weights, case.spec, **batch, **sw)
    w = cgnn_ref.split_keras_weights(case.weights, case.spec)
    ref = cgnn_ref.cgnn_forward(batch["y"], batch["pe"], batch["h_hat"], batch["active"], batch["mcs_mask"], w,
                                case.spec, num_it=sw.get("num_it"))
    for r, g in zip(ref["llr"], got["llr"]):
        assert np.abs(r - g).max() <= 1e-12 * max(1.0, np.abs(r).max())
    assert np.abs(ref["h_hat"] - got["h_ref"]).max() <= 1e-12 * max(1.0, np.abs(ref["h_hat"]).max())


def test_gradient_against_central_differences():
    """about 30 elements, one per array spread over the Keras list (every tensor kind: depthwise, pointwise, bias,
    dense), each drawn among the upper half of its array by |gradient| -- a relative error says nothing on an
    element whose derivative is rounding noise.  Step 1e-5: the rounding of the two losses (1e-16 / step) stays
    below 1e-6 of a derivative of 1e-4, and the step is small enough that no ReLU changes side between the two
    evaluations on this seed (a kink inside the step costs about 1 / (positions x units) = 1e-5 relative)."""
    case = make_case("nrx_rt", batch=1, users=2, prbs=1, active=[[1, 1]], seeded_weights=True)
    case.y, case.pe, case.h_hat = case.y[:, :3], case.pe[:, :3], case.h_hat[:, :, :3]      # F = 3: 84 positions
    batch = train_ref.training_batch(case)
    kw = dict(multiloss=True, w_chest=0.5)
    w = [np.asarray(a, np.float64) for a in case.weights]
    res = train_ref.loss_and_grad(w, case.spec, **batch, **kw)
    rng = np.random.default_rng(5)
    step, worst = 1e-5, 0.0
    for i in np.unique(np.linspace(0, len(w) - 1, 30).round().astype(int)):
        g = res["grads"][i].ravel()
        top = np.argsort(-np.abs(g))[:max(1, g.size // 2)]
        e = int(rng.choice(top))
        total = []
        for sgn in (1.0, -1.0):
            wp = [a.copy() for a in w]
            wp[i].ravel()[e] += sgn * step
            r = train_ref.loss_and_grad(wp, case.spec, **batch, **kw)
            total.append(r["loss_data"] + kw["w_chest"] * r["loss_chest"])
        fd = (total[0] - total[1]) / (2 * step)
        err = abs(fd - g[e]) / abs(g[e])
        worst = max(worst, err)
        assert err <= 1e-6, (i, e, fd, g[e])
    print(f"worst relative difference {worst:.2e}")


def test_loss_normalisation_by_hand():
    """constant LLR z on every RE, all bits 0: l = softplus(z); the mean counts inactive and other-MCS users"""
    case = make_case("nrx_rt_var_mcs", batch=2, users=2, prbs=1)
    sp = case.spec                                      # bits (2, 4)
    B, U, F, T, z, c = 2, 2, 12, 14, 0.7, 0.25
    active = torch.tensor([[1.0, 1.0], [1.0, 0.0]], dtype=torch.float64)
    mask = torch.zeros(B, U, 2, dtype=torch.float64)
    mask[0, 0, 0] = mask[0, 1, 1] = mask[1, 0, 1] = mask[1, 1, 0] = 1.0
    bits = torch.zeros(B, U, F, T, 4, dtype=torch.uint8)
    h = torch.zeros(B, U, F, T, 8, dtype=torch.float64)
    llrs = [torch.full((B, U, F, T, nb), z, dtype=torch.float64) for nb in sp.bits]
    ld, lc = train_ref.losses([(llrs, h + c)], sp, active, mask, bits, h, (2, 11))
    softplus = np.log1p(np.exp(z))
    # MCS 0: one active (slot, user) of four; MCS 1: two of four; the DMRS symbols drop out of both sides
    assert abs(float(ld) - (0.25 + 0.5) * softplus) < 1e-14
    assert abs(float(lc) - 0.75 * c * c) < 1e-14
    # bit 1 turns l into softplus(-z); two readouts add
    bits[...] = 1
    ld2, _ = train_ref.losses([(llrs, h)] * 2, sp, active, mask, bits, None, (2, 11))
    assert abs(float(ld2) - 2 * 0.75 * np.log1p(np.exp(-z))) < 1e-14


def test_adam_is_keras_adam():
    w, g = np.array([1.0, -2.0]), np.array([0.5, 0.0])
    w1, m1, v1 = train_ref.adam_step(w, g, np.zeros(2), np.zeros(2), 1)
    assert np.allclose(m1, [0.05, 0.0]) and np.allclose(v1, [0.00025, 0.0])
    assert np.allclose(w1, [1.0 - 1e-3 * 0.5 / (0.5 + 1e-7), -2.0], rtol=0, atol=1e-15)


def test_fixed_batch_trajectory_decreases():
    """the condition tests/test_gpu_train.py puts on the kernels holds for the reference alone"""
    case, batch = trajectory_case()
    total, _ = train_ref.trajectory(case.weights, case.spec, batch, TRAJ_STEPS, TRAJ_W_CHEST)
    print("total loss:", " ".join(f"{t:.6f}" for t in total))
    assert all(b < a for a, b in zip(total, total[1:])), total
