"""nrx_train_grad_acc on the GPU: one step's gradient from micro-batches, and checkpoint / resume (needs an MI355X).

The gate is that of tests/test_gpu_train.py, unchanged: per weight tensor ||g - g64|| / ||g64|| against the float64
autograd gradient of the WHOLE batch must stay within 4 max(e32, 1e-6), e32 being the worst tensor of the same
oracle run in float32 on the whole batch; both losses within 1e-6 relative of float64; exact zeros stay exact.

The inputs.  That gate presumes that float32 and float64 take the same side of every ReLU: a unit whose
pre-activation lies within float32 rounding of zero gets its backward mask from the summation order, and one such
unit moves whole weight tensors by 1e-3 (at ``make_case``'s default seed the single whole-batch call, split or not,
is 1.8e-3 from float64 in every tensor below the second iteration's aggregation MLP, while the splits agree with the
single call to 9e-8: slot 0 has a pre-activation 4e-8 of its layer's rms from zero).  So the random inputs are those
of the first ``make_case`` seed for which every ReLU pre-activation of the float64 oracle -- every readout included,
for the plain batch and the Var-IO batch alike -- is at least ``RELU_MARGIN`` = sqrt(128 + 9) 2^-24 = 7e-7 of its
layer's rms away from zero, the rounding of the longest sum that feeds a ReLU (128 pointwise terms of 9 taps each).
The criterion reads the oracle alone; ``test_inputs_have_no_relu_tie`` holds the inputs to it.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import train_ref
from tests.helpers import make_case
from tests.memguard import Guarded, same_bits
from tests.test_gpu_train import on_device, tensor_errors
from tests.test_train_ref import trajectory_case

pytestmark = pytest.mark.gpu

W_CHEST = 0.02
ACTIVITY = [[1, 1], [1, 0], [1, 1]]
RELU_MARGIN = float(np.sqrt(128 + 9) * 2.0 ** -24)
INPUT_SEED = 11         # the first seed whose margins (plain 1.9e-6, Var-IO 8.0e-7) both reach RELU_MARGIN


def relu_margin(case, batch):
    """min over every ReLU of the float64 oracle forward (all readouts) of |pre-activation| / rms of its layer"""
    real, worst = torch.relu, [np.inf]

    def spy(z):
        worst[0] = min(worst[0], float(z.abs().min() / z.pow(2).mean().sqrt()))
        return real(z)

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)   # noqa: E731
    torch.relu = spy
    try:
        with torch.no_grad():
            train_ref.forward([t(a) for a in case.weights], case.spec, t(batch["y"]), t(batch["pe"]), t(batch["h_hat"]),
                              t(batch["active"]), t(batch["mcs_mask"]), None, all_states=True)
    finally:
        torch.relu = real
    return worst[0]


def slice_batch(batch, lo, hi):
    """slots lo..hi-1 of a ``train_ref.training_batch`` (pe has no slot axis)"""
    return {k: (v if k == "pe" or v is None else np.ascontiguousarray(v[lo:hi])) for k, v in batch.items()}


def pieces_of(batch, sizes):
    out, lo = [], 0
    for n in sizes:
        out.append(on_device(slice_batch(batch, lo, lo + n)))
        lo += n
    assert lo == batch["active"].shape[0]
    return out


def run_split(case, batch, sw, sizes, own_denominator=False):
    """The batch as micro-batches of ``sizes`` slots: the first call overwrites a NaN-filled ``g`` and ``loss``,
    the others accumulate, ``batch_total`` = the whole batch (``own_denominator``: each call's own B).  Every call
    runs in a NaN-filled workspace of exactly the size asked for, with guard bands.  -> (gradients, loss, g bits)"""
    from neural_rx_amd.train import Trainer
    tr = Trainer(case.spec, case.weights)
    tr.g.fill_(float("nan"))
    tr.loss.fill_(float("nan"))
    total = sum(sizes)
    for i, ((sb, pe), n) in enumerate(zip(pieces_of(batch, sizes), sizes)):
        io = tr._io(sb, pe, sw.get("num_it"), sw.get("multiloss", False), sw.get("w_chest", 0.0), (2, 11))
        ws = Guarded(tr.workspace_bytes(io), 0xFF)
        tr.grad_async(sb, pe, workspace=ws.body, accumulate=i > 0, batch_total=n if own_denominator else total, **sw)
        torch.cuda.synchronize()
        ws.check(f"micro-batch {i} of {sizes}: training workspace")
    return tr.gradients(), tr.loss.tolist(), tr.g.cpu().numpy()


_CASES = {}


def whole(name):
    """(case, batch, switches, float64 result, float32 result) of a whole batch, computed once, never written to"""
    if name not in _CASES:
        if name == "vario":
            case = make_case(config="nrx_rt_var_mcs", batch=2, users=2, prbs=1, mcs_choice=[[0, 1], [1, 0]],
                             seed=INPUT_SEED)
            assert case.mcs_mask[..., 0].any() and case.mcs_mask[..., 1].any()       # both MCS present
            sw = dict(w_chest=W_CHEST)
        else:
            case = make_case(config="nrx_rt", batch=3, users=2, prbs=1, active=ACTIVITY, seed=INPUT_SEED)
            sw = dict(w_chest=W_CHEST, multiloss=name == "multiloss")
        batch = train_ref.training_batch(case)
        ref = train_ref.loss_and_grad(case.weights, case.spec, **batch, **sw)
        ref32 = train_ref.loss_and_grad(case.weights, case.spec, **batch, **sw, dtype=torch.float32)
        _CASES[name] = (case, batch, sw, ref, ref32)
    return _CASES[name]


@pytest.mark.parametrize("name", ["plain", "vario"])
def test_inputs_have_no_relu_tie(name):
    case, batch, _, _, _ = whole(name)
    margin = relu_margin(case, batch)
    print(f"{name}: smallest ReLU pre-activation {margin:.2e} of its layer's rms, required {RELU_MARGIN:.2e}")
    assert margin >= RELU_MARGIN


def gate(name, grads, loss, ref, ref32):
    e32 = max(tensor_errors(ref32["grads"], ref["grads"]))
    errs = tensor_errors(grads, ref["grads"])
    bound = 4 * max(e32, 1e-6)
    print(f"{name}: worst tensor {max(errs):.2e}  e32 {e32:.2e}  ratio to the bound {max(errs) / bound:.3f}  "
          f"loss {loss[0]:.7f} {loss[1]:.7f}  f64 {ref['loss_data']:.7f} {ref['loss_chest']:.7f}")
    return max(errs), bound


@pytest.mark.parametrize("name,splits", [("plain", [(1, 2), (2, 1)]), ("multiloss", [(1, 2), (2, 1)]),
                                         ("vario", [(1, 1)])])
def test_split_equals_whole(name, splits):
    case, batch, sw, ref, ref32 = whole(name)
    assert ref["loss_chest"] > 0
    for sizes in splits:
        grads, loss, bits = run_split(case, batch, sw, sizes)
        worst, bound = gate(f"{name} {sizes}", grads, loss, ref, ref32)
        assert all(np.isfinite(g).all() for g in grads)
        assert worst <= bound, (sizes, worst, bound)
        assert abs(loss[0] - ref["loss_data"]) <= 1e-6 * abs(ref["loss_data"])
        assert abs(loss[1] - ref["loss_chest"]) <= 1e-6 * abs(ref["loss_chest"])
        for i, (g, r) in enumerate(zip(grads, ref["grads"])):
            assert not g[r == 0].any(), i
        # the same sequence again: the same bits
        _, loss2, bits2 = run_split(case, batch, sw, sizes)
        assert same_bits(bits, bits2) and loss == loss2


def test_without_batch_total_it_is_wrong():
    """the 1 + 2 split with every call's own B in the denominators is not the gradient of the whole batch: the gate
    can tell"""
    case, batch, sw, ref, ref32 = whole("plain")
    grads, loss, _ = run_split(case, batch, sw, (1, 2), own_denominator=True)
    worst, bound = gate("own denominators (1, 2)", grads, loss, ref, ref32)
    assert worst > bound
    assert abs(loss[0] - ref["loss_data"]) > 1e-6 * abs(ref["loss_data"])


def test_unused_iterations_stay_zero_through_a_sequence():
    case, batch, _, _, _ = whole("plain")
    sw = dict(w_chest=W_CHEST, num_it=1)
    ref = train_ref.loss_and_grad(case.weights, case.spec, **batch, **sw)
    grads, loss, _ = run_split(case, batch, sw, (1, 1, 1))
    unused = [i for i, r in enumerate(ref["grads"]) if not r.any()]
    assert len(unused) >= 13
    for i in unused:
        assert not grads[i].any() and not np.signbit(grads[i]).any()
    assert abs(loss[0] - ref["loss_data"]) <= 1e-6 * abs(ref["loss_data"])


def test_identity_with_train_grad():
    """acc = NULL, accumulate = 0 with batch_total = B onto a NaN-filled grad, accumulate = 1 with batch_total = B
    onto zeroed buffers: the bits of nrx_train_grad"""
    from neural_rx_amd import _lib
    from neural_rx_amd.train import Trainer
    name = next(iter(train_ref.CASES))
    case, batch, sw = train_ref.build_case(name)
    assert batch["active"].shape == (2, 2) and batch["y"].shape[1] == 12
    sb, pe = on_device(batch)
    tr = Trainer(case.spec, case.weights)
    tr.g.fill_(float("nan"))
    tr.grad_async(sb, pe, w_chest=W_CHEST, **sw)
    want = (tr.g.cpu().numpy(), tr.loss.cpu().numpy())
    assert np.isfinite(want[0]).all() and want[1][0] > 0 and want[1][1] > 0
    B = 2

    def call(acc, fill):
        tr.g.fill_(fill)
        tr.loss.fill_(fill)
        io = tr._io(sb, pe, sw.get("num_it"), sw.get("multiloss", False), W_CHEST, (2, 11))
        ws = Guarded(tr.workspace_bytes(io), 0xFF)
        _lib.check(tr._lib.nrx_train_grad_acc(ctypes.byref(tr._desc), ctypes.byref(io),
                                              ctypes.byref(acc) if acc is not None else None, ws.body.data_ptr(),
                                              ws.body.numel(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        ws.check("training workspace")
        return tr.g.cpu().numpy(), tr.loss.cpu().numpy()

    for what, acc, fill in (("NULL", None, float("nan")), ("overwrite", _lib.nrx_train_acc(0, B), float("nan")),
                            ("accumulate onto zeros", _lib.nrx_train_acc(1, B), 0.0)):
        g, loss = call(acc, fill)
        assert same_bits(g, want[0]) and same_bits(loss, want[1]), what
    # ... and through the wrapper
    tr.g.fill_(float("nan"))
    tr.grad_async(sb, pe, w_chest=W_CHEST, batch_total=B, **sw)
    assert same_bits(tr.g.cpu().numpy(), want[0])


def test_grad_micro_is_the_sequence_of_calls():
    from neural_rx_amd.train import Trainer
    case, batch, sw, ref, ref32 = whole("plain")
    _, loss, bits = run_split(case, batch, sw, (1, 2))
    tr = Trainer(case.spec, case.weights)
    tr.g.fill_(float("nan"))
    pieces = pieces_of(batch, (1, 2))
    tr.grad_micro([sb for sb, _ in pieces], pieces[0][1], **sw)
    assert same_bits(tr.g.cpu().numpy(), bits) and tr.loss.tolist() == loss
    # one workspace, that of the largest micro-batch
    io = tr._io(pieces[1][0], pieces[1][1], None, False, W_CHEST, (2, 11))
    assert tr._ws.buf.numel() == tr.workspace_bytes(io)


def test_resume_repeats_the_uninterrupted_run(tmp_path):
    from neural_rx_amd import weights as W
    from neural_rx_amd.train import Trainer
    case, batch = trajectory_case()
    sb, pe = on_device(batch)

    def steps(tr, n):
        for _ in range(n):
            tr.grad_async(sb, pe, w_chest=W_CHEST)
            tr.step()

    straight = Trainer(case.spec, case.weights)
    steps(straight, 4)
    first = Trainer(case.spec, case.weights)
    steps(first, 2)
    path = str(tmp_path / "run.state.npz")
    first.save_state(path, global_step=2)
    assert all(same_bits(a, b) for a, b in zip(W.load_file(path), first.weights()))     # still a weight file
    second = Trainer(case.spec, W.seeded(case.spec, seed=99))                           # other weights: all restored
    assert second.load_state(path) == 2 and second.num_steps == 2
    steps(second, 2)
    assert second.num_steps == straight.num_steps == 4
    for name in ("w", "m", "v"):
        a, b = getattr(second, name).cpu().numpy(), getattr(straight, name).cpu().numpy()
        assert same_bits(a, b), name
    assert not same_bits(first.w.cpu().numpy(), straight.w.cpu().numpy())                # the last two steps moved w
    W.save(str(tmp_path / "w.npz"), first.weights())
    with pytest.raises(ValueError, match="optimizer state"):
        second.load_state(str(tmp_path / "w.npz"))
