"""Oracle of the training path (test infrastructure, CPU): the CGNN forward of ``oracle/cgnn_torch.py`` restated
with autograd on, the loss of include/nrx.h (``nrx_train_io``) and Keras Adam in numpy.

The forward is the one of ``oracle/cgnn_torch.py`` on parameters kept in their Keras shapes, so the gradients come
back as the Keras-ordered list.  One difference: the depthwise 3x3 is the nine shifted multiply-adds of
``oracle/cgnn_ref.py: sepconv``, not a grouped ``conv2d``.  In float64 the two agree to rounding; in float32 the CPU
``conv2d`` is not an exact-float32 computation for every shape (B = 2, U = 2, 1 PRB: gradients 2e-3 from float64
where the shifted form is 3e-7 away), and the float32 run of this oracle is the yardstick of the GPU gate.
Loss, with LLR > 0 meaning bit 1:

  loss_data  = sum_r sum_m [ sum active[b,u] mask[b,u,m] l(z, bit) ] / (B U F (14 - n_dmrs) bits_m)
               l = max(z, 0) - bit z + log1p(exp(-|z|)) over data symbols and the bits k < bits_m
  loss_chest = sum_r mean over [B,U,F,T,2A] of active[b,u] (h_ref - h)^2
  total      = loss_data + w_chest loss_chest

over the readouts r: after the last iteration, or with ``multiloss`` after every iteration.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import cgnn_ref


def _sep_stack(z, layers):
    """z [N, F, T, C]; layers: 3 x (dw [3,3,C,1], pw [1,1,C,Co], b [Co]) in Keras shapes"""
    for k, (dw, pw, b) in enumerate(layers):
        f, t = z.shape[1], z.shape[2]
        zp = Fn.pad(z, (0, 0, 1, 1, 1, 1))
        d = 0
        for i in range(3):
            for j in range(3):
                d = d + dw[i, j, :, 0] * zp[:, i:i + f, j:j + t, :]
        z = d @ pw[0, 0] + b
        if k < len(layers) - 1:
            z = torch.relu(z)
    return z


def _dense2(x, layers):
    (w1, b1), (w2, b2) = layers
    return torch.relu(x @ w1 + b1) @ w2 + b2


def forward(params: List[torch.Tensor], spec, y, pe, h_hat, active, mcs_mask, num_it=None, all_states=False):
    """``params``: the Keras-ordered list as tensors.  Returns the list of states read out (the last one, or
    with ``all_states`` the one after every iteration) as ``[(llrs per MCS, h_ref)]``."""
    w = cgnn_ref.split_keras_weights(params, spec)         # only groups the list: works on tensors
    sep = lambda ls: [(l.dw, l.pw, l.b) for l in ls]       # noqa: E731
    den = lambda ls: [(l.w, l.b) for l in ls]              # noqa: E731
    num_it = spec.num_it if num_it is None else num_it
    B, F, T, _ = y.shape
    U = pe.shape[0]
    ms = (y * y).mean(dim=(1, 2, 3))
    ns = torch.where(ms > 0, 1.0 / torch.sqrt(torch.where(ms > 0, ms, torch.ones_like(ms))), torch.zeros_like(ms))
    parts = [(y * ns[:, None, None, None])[:, None].expand(B, U, F, T, y.shape[-1]), pe[None].expand(B, U, F, T, 2)]
    if h_hat is not None:
        parts.append(h_hat * ns[:, None, None, None, None])
    z0 = torch.cat(parts, dim=-1).reshape(B * U, F, T, -1)
    if spec.masking:
        s = _sep_stack(z0, sep(w.init[0]))
    else:
        s = sum(_sep_stack(z0, sep(w.init[m])) * mcs_mask.reshape(B * U, -1)[:, m, None, None, None]
                for m in range(spec.num_init))
    s = s.reshape(B, U, F, T, -1)
    act = active.reshape(B, U, 1, 1, 1)
    p = (active.sum(dim=1) - 1.0).clamp_min(0.0)
    p = torch.where(p == 0, torch.ones_like(p), 1.0 / torch.where(p == 0, torch.ones_like(p), p))
    pe_t = pe[None].expand(B, U, F, T, 2)

    def readout(s):
        llrs = []
        for m in range(spec.num_mcs):
            out = _dense2(s, den(w.llr[0 if spec.masking else m]))
            llrs.append(out[..., :spec.bits[m]])
        return llrs, _dense2(s, den(w.chest))

    outs = []
    for i in range(num_it):
        sp_ = _dense2(s, den(w.agg[i])) * act
        a = (sp_.sum(dim=1, keepdim=True) - sp_) * p[:, None, None, None, None]
        z = torch.cat([a, s, pe_t], dim=-1).reshape(B * U, F, T, -1)
        s = _sep_stack(z, sep(w.update[i])).reshape(B, U, F, T, -1) + s
        if all_states or i == num_it - 1:
            outs.append(readout(s))
    return outs


class _StableBCE(torch.autograd.Function):
    """l(z, bit) with the derivative formed without cancellation: sigmoid(z) for bit 0, -sigmoid(-z) for bit 1,
    each from e = exp(-|z|) as e / (1 + e) on its small side and 1 / (1 + e) on its large one.  Autograd on the
    three terms of l gives the same number in float64; in float32 it adds 1 - bit and -+ e / (1 + e) in whatever
    order the graph has, and at a confident, correct LLR (the derivative is the small side, 1e-5) that costs digits."""

    @staticmethod
    def forward(ctx, z, bit):
        ctx.save_for_backward(z, bit)
        return z.clamp_min(0) - bit * z + torch.log1p(torch.exp(-z.abs()))

    @staticmethod
    def backward(ctx, g):
        z, bit = ctx.saved_tensors
        e = torch.exp(-z.abs())
        big, small = 1.0 / (1.0 + e), e / (1.0 + e)
        d = torch.where(bit != 0, -torch.where(z >= 0, small, big), torch.where(z >= 0, big, small))
        return g * d, None


def losses(outs, spec, active, mcs_mask, bits, h, dmrs_symbols, stable_loss=False):
    """(loss_data, loss_chest) of the readouts ``outs`` of ``forward``; ``h`` None: loss_chest = 0.
    ``stable_loss``: the derivative of l by ``_StableBCE``, not by autograd on its terms"""
    B, U, F, T = bits.shape[:4]
    data = [t for t in range(T) if t not in set(dmrs_symbols)]
    ld = torch.zeros((), dtype=active.dtype)
    lc = torch.zeros((), dtype=active.dtype)
    for llrs, h_ref in outs:
        for m, z in enumerate(llrs):
            nb = spec.bits[m]
            z = z[:, :, :, data]
            bit = bits[:, :, :, data, :nb].to(z.dtype)
            ell = _StableBCE.apply(z, bit) if stable_loss else \
                z.clamp_min(0) - bit * z + torch.log1p(torch.exp(-z.abs()))
            wgt = (active * mcs_mask[:, :, m])[:, :, None, None, None]
            ld = ld + (wgt * ell).sum() / (B * U * F * len(data) * nb)
        if h is not None:
            lc = lc + (active[:, :, None, None, None] * (h_ref - h) ** 2).mean()
    return ld, lc


def loss_and_grad(weights: Sequence[np.ndarray], spec, y, pe, h_hat, active, mcs_mask, bits, h,
                  dmrs_symbols=(2, 11), num_it=None, multiloss=False, w_chest=0.0, dtype=torch.float64,
                  stable_loss=False):
    """The losses, the Keras-ordered gradient list of ``loss_data + w_chest loss_chest`` (zeros for the arrays of
    unused iterations) and the last readout, all numpy.  ``mcs_mask`` None: one-hot on MCS 0.  ``bits`` may be
    wider than ``bits_max``: the columns beyond are not labels.  ``stable_loss``: see ``losses``."""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)     # noqa: E731
    params = [t(a).requires_grad_(True) for a in weights]
    B, U = active.shape
    if mcs_mask is None:
        mcs_mask = np.zeros((B, U, spec.num_mcs), np.float32)
        mcs_mask[..., 0] = 1.0
    act, mask = t(active), t(mcs_mask)
    outs = forward(params, spec, t(y), t(pe), t(h_hat), act, mask, num_it, all_states=multiloss)
    ld, lc = losses(outs, spec, act, mask, torch.from_numpy(np.ascontiguousarray(bits)), t(h), dmrs_symbols,
                    stable_loss)
    (ld + w_chest * lc).backward()
    grads = [np.zeros(a.shape, a.detach().numpy().dtype) if a.grad is None else a.grad.numpy() for a in params]
    llrs, h_ref = outs[-1]
    return dict(loss_data=float(ld.detach()), loss_chest=float(lc.detach()), grads=grads, llr=[z.detach().numpy() for z in llrs],
                h_ref=h_ref.detach().numpy())


def adam_step(w, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """Keras Adam on arrays of any float type: the new (w, m, v)"""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    w = w - lr * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)
    return w, m, v


def adam_step_f32(w, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """the same on float32 state, formed in float64: m and v are rounded to float32 as they are stored, and the
    update of w reads the stored values (what ``nrx_adam_step`` documents)"""
    g = g.astype(np.float64)
    m = (b1 * m.astype(np.float64) + (1 - b1) * g).astype(np.float32)
    v = (b2 * v.astype(np.float64) + (1 - b2) * g * g).astype(np.float32)
    w = w.astype(np.float64) - lr * (m.astype(np.float64) / (1 - b1 ** t)) / (np.sqrt(v.astype(np.float64) / (1 - b2 ** t)) + eps)
    return w.astype(np.float32), m, v


def trajectory(weights, spec, batch, steps, w_chest, dtype=torch.float64, **kw):
    """``steps`` Adam steps on one fixed batch (``batch``: the keyword arguments of ``loss_and_grad``): the total
    loss before every step and after the last, and the final weights"""
    np_t = np.float64 if dtype == torch.float64 else np.float32
    w = [np.asarray(a, np_t) for a in weights]
    m = [np.zeros_like(a) for a in w]
    v = [np.zeros_like(a) for a in w]
    total = []
    for t in range(1, steps + 2):
        r = loss_and_grad(w, spec, w_chest=w_chest, dtype=dtype, **batch)
        total.append(r["loss_data"] + w_chest * r["loss_chest"])
        if t > steps:
            break
        for i, g in enumerate(r["grads"]):
            w[i], m[i], v[i] = adam_step(w[i], g.astype(np_t), m[i], v[i], t, **kw)
            w[i], m[i], v[i] = w[i].astype(np_t), m[i].astype(np_t), v[i].astype(np_t)
    return total, w


# The gradient cases: every topology path of nrx_train_grad at the smallest grid (1 PRB = 168 positions per
# (slot, user)).  name -> (tests.helpers.make_case arguments, nrx_train_io switches)
CASES = {
    "rt_b2_u2": (dict(config="nrx_rt", batch=2, users=2, prbs=1, active=[[1, 1], [1, 0]]), {}),
    "rt_b3_u1": (dict(config="nrx_rt", batch=3, users=1, prbs=1), {}),                        # P = 504
    "rt_b2_u3": (dict(config="nrx_rt", batch=2, users=3, prbs=1, active=[[1, 1, 1], [1, 0, 1]]), {}),
    "rt_2prb": (dict(config="nrx_rt", batch=2, users=2, prbs=2), {}),
    "var_mcs": (dict(config="nrx_rt_var_mcs", batch=2, users=2, prbs=1, mcs_choice=[[0, 1], [1, 0]]), {}),
    # The masked head on the shipped weights at 2 of their 8 iterations, and all 8 on seeded weights.  Not the
    # shipped weights at full depth: there float32 itself is 1e-3 from float64 (ReLUs that take the other side;
    # LLRs reach 73 on random labels) and the CPU float32 figure moves by an order of magnitude from one machine
    # to the next (1.2e-4 to 1.5e-3 measured), so 4 e32 is no stable bound (DESIGN.md section 9 has the figures).
    "masked": (dict(config="nrx_large_var_mcs_64qam_masking", batch=2, users=2, prbs=1,
                    mcs_choice=[[0, 2], [1, 0]]), dict(num_it=2)),
    "masked_8it_seeded": (dict(config="nrx_large_var_mcs_64qam_masking", batch=2, users=2, prbs=1,
                               mcs_choice=[[0, 2], [1, 0]], seeded_weights=True), {}),
    "odd_a_no_h": (dict(config="nrx_rt", batch=2, users=2, prbs=1, num_rx_ant=3, no_h_hat=True), {}),
    "rt_multiloss": (dict(config="nrx_rt", batch=2, users=2, prbs=1, active=[[1, 1], [1, 0]]),
                     dict(multiloss=True, w_chest=0.5)),
    "rt_num_it_1": (dict(config="nrx_rt", batch=2, users=2, prbs=1, active=[[1, 1], [1, 0]]), dict(num_it=1)),
}


def build_case(name):
    """``(case, batch, switches)``: a ``tests.helpers`` case, its ``training_batch`` and the switches"""
    import dataclasses
    from neural_rx_amd import weights as W
    from tests.helpers import make_case
    kw, sw = CASES[name]
    kw = dict(kw)
    if kw.pop("no_h_hat", False):       # seeded weights: no trained set has 3 antennas or lacks h_hat
        case = make_case(random_inputs=True, seeded_weights=True, **kw)
        case.spec = dataclasses.replace(case.spec, use_h_hat=False)
        case.weights = W.seeded(case.spec, seed=3)
        case.h_hat = None
    else:
        case = make_case(**kw)
    return case, training_batch(case), dict(sw)


def training_batch(case, seed=0):
    """labels for a ``tests.helpers`` case: random bits ``[B,U,F,14,bits_max]`` and a true channel ``h``; the
    keyword arguments of ``loss_and_grad``"""
    rng = np.random.default_rng(seed + 1000)
    B, U = case.active.shape
    F = case.y.shape[1]
    sp = case.spec
    bits = rng.integers(0, 2, size=(B, U, F, 14, sp.bits_max)).astype(np.uint8)
    h = rng.standard_normal((B, U, F, 14, 2 * sp.num_rx_ant)).astype(np.float32)
    return dict(y=case.y, pe=case.pe, h_hat=case.h_hat if sp.use_h_hat else None, active=case.active,
                mcs_mask=case.mcs_mask, bits=bits, h=h)


# ---------------------------------------------------------------- the cases beyond the first corner
def slab_positions(P, max_slabs=256):
    """PC of nrx_train.hip ``make_plan``: the positions one workgroup of k_wgrad / k_dwgrad reduces, P spread over
    at most ``max_slabs`` (kMaxSlabs) chunks and rounded up to the 32-position step"""
    return ((P + max_slabs - 1) // max_slabs + 31) // 32 * 32


def topo_activity(users):
    """three slots: every user active, the last one alone, every user but the last (U = 2: [[1,1],[0,1],[1,0]]):
    a slot with two or more active users, one with exactly one, an inactive (slot, user)"""
    act = np.ones((3, users), np.float32)
    act[1, :-1] = 0
    act[2, -1] = 0
    return act


def _seeded_rt(name, batch, F, active, seed=7):
    """the nrx_rt topology on seeded weights, U = 2, random inputs on an F-subcarrier grid (F = 1: the first
    subcarrier of the F = 2 grid, the second user's pilots lying on odd subcarriers)"""
    from tests.test_gpu_topologies import topo_case
    case = topo_case({}, 2, max(F, 2), batch, seed, active=active, name=name)
    if F < 2:
        case.y, case.pe, case.h_hat = (np.ascontiguousarray(a) for a in (case.y[:, :F], case.pe[:, :F], case.h_hat[:, :, :F]))
    return case


def _topo(name):
    from tests.test_gpu_topologies import SEEDS, TOPOLOGIES, VARIO_A4, topo_case
    t = VARIO_A4 if name == "vario_a4" else TOPOLOGIES[name]
    U = t["users"]
    mask = "soft" if name == "a6_mask8_u16" else t.get("mask")
    case = topo_case(t["spec"], U, 5, 3, SEEDS.get(name, 11), active=topo_activity(U) if U >= 2 else None,
                     mcs_mask=mask, name=name)
    sw = dict(w_chest=0.5)
    if "run_it" in t:
        sw["num_it"] = t["run_it"]
    if name in ("a6_mask8_u16", "a3_noh_3heads_u5"):
        sw["multiloss"] = True
    return case, training_batch(case), sw, {}


def _slab64(name):
    from tests.helpers import make_case
    active = np.ones((9, 3), np.float32)
    active[4, 1] = 0
    case = make_case(config="nrx_rt", batch=9, users=3, prbs=2, active=active)
    return case, training_batch(case), dict(w_chest=0.02), {}


def _grid(F):
    def build(name):
        case = _seeded_rt(name, 2, F, [[1, 1], [1, 0]])
        return case, training_batch(case), dict(w_chest=0.5), {}
    return build


def _dmrs(symbols):
    def build(name):
        case = _seeded_rt(name, 2, 5, [[1, 1], [0, 1]])
        return case, training_batch(case), dict(w_chest=0.5, dmrs_symbols=tuple(symbols)), {}
    return build


def _none_mask_vario(name):
    from tests.test_gpu_topologies import VARIO_A4, topo_case
    case = topo_case(VARIO_A4["spec"], 2, 5, 3, 11, active=topo_activity(2), name=name)
    return case, dict(training_batch(case), mcs_mask=None), dict(w_chest=0.5), {}


def _none_mask_masked(name):
    from tests.helpers import make_case
    case = make_case(config="nrx_large_var_mcs_64qam_masking", batch=2, users=2, prbs=1, active=[[1, 1], [1, 0]],
                     seeded_weights=True)
    return case, dict(training_batch(case), mcs_mask=None), dict(num_it=2, w_chest=0.5), {}


def _bits_wide(name):
    case = _seeded_rt(name, 2, 5, [[1, 1], [1, 0]])
    batch = training_batch(case)
    B, U, F, T, nb = batch["bits"].shape
    batch["bits"] = np.concatenate([batch["bits"], np.ones((B, U, F, T, 11 - nb), np.uint8)], axis=-1)
    return case, batch, dict(w_chest=0.5), {}


def _dead_slots(name):
    """slot 1 is all zero (ns = 0) with one active user, slot 2 has no active user; ``alt``: the same batch with
    other labels (bits and h) in slot 2, which must not change anything"""
    case = _seeded_rt(name, 3, 5, [[1, 1], [1, 0], [0, 0]])
    case.y[1], case.h_hat[1] = 0, 0
    batch = training_batch(case)
    alt = dict(batch, bits=batch["bits"].copy(), h=batch["h"].copy())
    alt["bits"][2] ^= 1
    alt["h"][2] = 3.0 - 2.0 * alt["h"][2]
    return case, batch, dict(w_chest=0.5), dict(alt=alt)


CONFIDENT_SHIFT = 12.0


def _confident(name):
    """every LLR confident and correct: the head's last bias moved by +-12 (even / odd bit index) and the labels
    set to match, so that every derivative of l is the small side of the sigmoid"""
    case = _seeded_rt(name, 2, 5, [[1, 1], [1, 0]])
    nb = case.spec.bits_max
    sign = np.where(np.arange(nb) % 2 == 0, 1.0, -1.0).astype(np.float32)
    bias = case.weights[-5]                              # ..., head (w1, b1, w2, b2), ChEst (w1, b1, w2, b2)
    assert bias.shape == (nb,)
    case.weights[-5] = bias + CONFIDENT_SHIFT * sign
    batch = training_batch(case)
    batch["bits"][...] = (sign > 0).astype(np.uint8)
    return case, batch, dict(w_chest=0.0), dict(stable32=True)


TOPO_NAMES = ("a1_qpsk_u1", "a3_noh_3heads_u5", "a4_noh_u2", "a6_mask8_u16", "a8_64qam_u3", "a9_b5_u7", "vario_a4")
# name -> builder(name) of (case, batch, switches, extras); extras: stable32 (the float32 yardstick is the
# oracle with the cancellation-free loss derivative), alt (a second batch the test compares with)
MORE_CASES = {
    "rt_slab64": _slab64,                                # P = 9072: PC = 64, two steps per chunk, a 16-row tail
    **{"topo_" + n: (lambda name, n=n: _topo(n)) for n in TOPO_NAMES},
    "grid_f1": _grid(1), "grid_f2": _grid(2), "grid_f13": _grid(13),
    "dmrs_2": _dmrs((2,)), "dmrs_2_3_10_11": _dmrs((2, 3, 10, 11)), "dmrs_0_13": _dmrs((0, 13)),
    "dmrs_0_to_12": _dmrs(range(13)),
    "none_mask_vario": _none_mask_vario, "none_mask_masked": _none_mask_masked,
    "bits_wide": _bits_wide, "dead_slots": _dead_slots, "confident": _confident,
}
_MORE, _REFS = {}, {}


def more_case(name):
    """``(case, batch, switches, extras)`` of ``MORE_CASES[name]``, built once; nobody writes to it"""
    if name not in _MORE:
        _MORE[name] = MORE_CASES[name](name)
    return _MORE[name]


def more_references(name):
    """``(float64 result, float32 result)`` of ``loss_and_grad`` on ``more_case(name)``, computed once"""
    if name not in _REFS:
        case, batch, sw, extras = more_case(name)
        ref = loss_and_grad(case.weights, case.spec, **batch, **sw)
        ref32 = loss_and_grad(case.weights, case.spec, **batch, **sw, dtype=torch.float32,
                              stable_loss=bool(extras.get("stable32")))
        _REFS[name] = (ref, ref32)
    return _REFS[name]
