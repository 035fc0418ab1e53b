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


# ---------------------------------------------------------------- the cases of tests/test_gpu_train_cases.py
def tensor_errors(grads, ref):
    """||g - ref|| / ||ref|| per array with a non-zero reference"""
    out = []
    for g, r in zip(grads, ref):
        n = np.linalg.norm(r)
        if n > 0:
            out.append(float(np.linalg.norm(np.asarray(g, np.float64) - r) / n))
    return out


def positions(batch):
    B, U, F = batch["bits"].shape[:3]
    return B * U * F * 14


def test_slab_case_takes_two_steps_and_a_tail():
    """rt_slab64 is the case whose k_wgrad loop runs more than once: PC from the documented formula"""
    _, batch, _, _ = train_ref.more_case("rt_slab64")
    P = positions(batch)
    PC = train_ref.slab_positions(P)
    assert (P, PC) == (9072, 64) and -(-P // PC) == 142
    assert P - 141 * PC == 48                           # the last chunk: one full step and a 16-row tail
    assert not batch["active"].all()
    assert train_ref.slab_positions(8192) == 32         # nothing smaller reaches the loop
    # every other case is a one-step one
    assert all(train_ref.slab_positions(positions(train_ref.more_case(n)[1])) == 32
               for n in train_ref.MORE_CASES if n != "rt_slab64")


def test_grid_edge_chunks_cross_the_slot_user_boundaries():
    _, batch, _, _ = train_ref.more_case("grid_f13")
    B, U, F = batch["bits"].shape[:3]
    assert all((bu * F * 14) % 32 for bu in range(1, B * U))


@pytest.mark.parametrize("name", [n for n in train_ref.TOPO_NAMES if n != "a1_qpsk_u1"])
def test_topology_cases_train_every_array(name):
    """a slot with two active users, one with exactly one, an inactive (slot, user) -- and with them no array of
    an iteration that runs has an all-zero gradient (the aggregation MLPs' were, under seeded activity)"""
    case, batch, sw, _ = train_ref.more_case("topo_" + name)
    n_act = batch["active"].sum(axis=1)
    assert (n_act >= 2).any() and (n_act == 1).any() and (batch["active"] == 0).any()
    ref, _ = train_ref.more_references("topo_" + name)
    sp = case.spec
    first = 9 * sp.num_init                             # the StateInit stacks, then 13 arrays per iteration
    unused = set(range(first + 13 * sw.get("num_it", sp.num_it), first + 13 * sp.num_it))
    zero = {i for i, g in enumerate(ref["grads"]) if not g.any()}
    assert zero == unused, sorted(zero ^ unused)


def test_single_user_topology_has_zero_aggregation_gradients():
    ref, _ = train_ref.more_references("topo_a1_qpsk_u1")
    zero = {i for i, g in enumerate(ref["grads"]) if not g.any()}
    assert zero == {9 + 13 * i + k for i in range(2) for k in range(4)}


def test_mask_fixtures():
    """soft rows on both masked-sum paths, a missing mask where the issue asks for one"""
    for name in ("topo_a3_noh_3heads_u5", "topo_a6_mask8_u16"):
        m = train_ref.more_case(name)[1]["mcs_mask"]
        hot = (m == 1).any(axis=-1)
        assert hot.any() and not hot.all() and ((m > 0).sum(axis=-1)[~hot] == m.shape[-1]).all()
    for name in ("none_mask_vario", "none_mask_masked"):
        assert train_ref.more_case(name)[1]["mcs_mask"] is None


def test_none_mask_zeroes_what_mcs_0_does_not_reach():
    # Var-IO: StateInit stack 1 and LLR head 1
    case, _, _, _ = train_ref.more_case("none_mask_vario")
    ref, _ = train_ref.more_references("none_mask_vario")
    n = len(ref["grads"])
    zero = {i for i, g in enumerate(ref["grads"]) if not g.any()}
    assert zero == set(range(9, 18)) | set(range(n - 8, n - 4))
    # the masked head: the columns >= bits_0 of its last dense layer, and nothing else of the iterations run
    case, _, sw, _ = train_ref.more_case("none_mask_masked")
    ref, _ = train_ref.more_references("none_mask_masked")
    nb = case.spec.bits[0]
    w2, b2 = ref["grads"][-6], ref["grads"][-5]
    assert w2.shape[1] == case.spec.bits_max > nb
    assert not w2[:, nb:].any() and not b2[nb:].any() and w2[:, :nb].any(axis=0).all() and b2[:nb].all()
    zero = {i for i, g in enumerate(ref["grads"]) if not g.any()}
    assert zero == set(range(9 + 13 * sw["num_it"], 9 + 13 * case.spec.num_it))


def test_wide_bits_and_dead_slot_labels_are_not_read():
    case, batch, sw, _ = train_ref.more_case("bits_wide")
    assert batch["bits"].shape[-1] == 11 > case.spec.bits_max and batch["bits"][..., case.spec.bits_max:].all()
    ref, _ = train_ref.more_references("bits_wide")
    narrow = dict(batch, bits=np.ascontiguousarray(batch["bits"][..., :case.spec.bits_max]))
    got = train_ref.loss_and_grad(case.weights, case.spec, **narrow, **sw)
    assert all(np.array_equal(a, b) for a, b in zip(ref["grads"], got["grads"]))
    case, batch, sw, extras = train_ref.more_case("dead_slots")
    assert not batch["y"][1].any() and not batch["h_hat"][1].any() and batch["active"][1].any()
    assert not batch["active"][2].any()
    alt = extras["alt"]
    assert (alt["bits"][2] != batch["bits"][2]).all() and (alt["h"][2] != batch["h"][2]).all()
    assert np.array_equal(alt["bits"][:2], batch["bits"][:2]) and np.array_equal(alt["h"][:2], batch["h"][:2])
    ref, _ = train_ref.more_references("dead_slots")
    got = train_ref.loss_and_grad(case.weights, case.spec, **alt, **sw)
    assert all(np.isfinite(g).all() for g in ref["grads"])
    assert all(np.array_equal(a, b) for a, b in zip(ref["grads"], got["grads"]))
    assert (ref["loss_data"], ref["loss_chest"]) == (got["loss_data"], got["loss_chest"])


def test_stable_loss_derivative():
    """float64: the cancellation-free derivative is autograd's to 1e-12 on random labels.  float32, every LLR confident and
    correct: autograd on the terms of l is more than 100 times further from float64 -- so a kernel that formed
    sigmoid(z) - bit would miss the bound the stable oracle sets"""
    case, batch, sw, extras = train_ref.more_case("confident")
    assert extras["stable32"] and sw["w_chest"] == 0.0
    ref, stable32 = train_ref.more_references("confident")
    z = ref["llr"][0]
    data = [t for t in range(14) if t not in (2, 11)]
    assert 11.0 <= np.abs(z).min() and np.abs(z).max() <= 13.0      # the seeded head itself stays within +-1
    assert ((z > 0) == (batch["bits"] != 0))[:, :, :, data].all()
    # here autograd cancels in float64 too: 2^-53 against derivatives down to sigmoid(-13) = 2e-6 is 5e-11
    stable64 = train_ref.loss_and_grad(case.weights, case.spec, **batch, **sw, stable_loss=True)
    assert max(tensor_errors(stable64["grads"], ref["grads"])) <= 1e-10
    plain32 = train_ref.loss_and_grad(case.weights, case.spec, **batch, **sw, dtype=torch.float32)
    e_plain = max(tensor_errors(plain32["grads"], ref["grads"]))
    e_stable = max(tensor_errors(stable32["grads"], ref["grads"]))
    print(f"worst tensor against float64: plain {e_plain:.2e}  stable {e_stable:.2e}")
    assert e_stable <= 1e-6 and e_plain > 100 * e_stable
    # on random labels, where nothing cancels, the two float64 gradients agree to 1e-12
    for name in ("grid_f2", "topo_vario_a4", "none_mask_masked"):
        case, batch, sw, _ = train_ref.more_case(name)
        ref, _ = train_ref.more_references(name)
        stable64 = train_ref.loss_and_grad(case.weights, case.spec, **batch, **sw, stable_loss=True)
        assert max(tensor_errors(stable64["grads"], ref["grads"])) <= 1e-12, name
