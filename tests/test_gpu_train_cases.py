"""nrx_train_grad beyond its first corner: slab loops, every topology, grid and loss edges, streams (needs an MI355X).

The ten cases of tests/train_ref.py ``CASES`` all have P <= 1344 positions (one 32-position step per k_wgrad
workgroup), the nrx_rt family's topologies, DMRS symbols (2, 11), ``bits_stride = bits_max`` and random labels.
``train_ref.MORE_CASES`` holds what that leaves out; every case goes through ``check_gradient_parity`` of
tests/test_gpu_train.py (per tensor ||g - g64|| / ||g64|| <= 4 max(e32, 1e-6), exact zeros, losses to 1e-6, LLR /
h_ref inside the f32X bounds), in a NaN-filled guarded workspace of exactly ``workspace_bytes(io)``.

  rt_slab64         nrx_rt shipped, B = 9, U = 3, 2 PRB: PC = 64, so every k_wgrad / k_dwgrad workgroup takes two
                    steps (accumulating MFMA results and bsum), the last one a full step and a 16-row tail
  topo_*            the six topologies of test_gpu_topologies.py and Var-IO over 2A = 8 at B = 3, F = 5 (F no
                    multiple of 12): 2A = 2 / 6 / 8 / 12 / 16 / 18 (C0 = 38: a k loop of 32 + 6), heads of 1 / 3 /
                    8 bits (K = 1 and K = 3 in bwd_data), 8 MCS on a masked head, U = 1 / 5 / 7 / 16, soft masks
                    on the per-MCS StateInit sum and on the masked head's sum over m, multiloss, w_chest = 0.5
  grid_f1/f2/f13    F = 1 (no frequency neighbour), F = 2, F = 13 (FT = 182: no chunk boundary on a (slot, user)
                    boundary, the k_dwgrad taps cross chunks on both sides)
  dmrs_*            dmrs_symbol_mask of (2,), (2, 3, 10, 11), (0, 13), (0 .. 12)
  none_mask_*       mcs_mask = NULL on Var-IO (StateInit 1 and head 1 get exact zeros) and on the 3-MCS masked
                    head (the columns >= bits_0 of its last layer do)
  bits_wide         bits rows of 11 (bits_stride > bits_max), the columns beyond the labels all 1
  dead_slots        an all-zero slot (ns = 0), a slot with no active user whose labels must not matter
  confident         every LLR at +-12 and correct: the derivative is the small side of the sigmoid everywhere;
                    e32 is the float32 oracle with the cancellation-free derivative (plain float32 autograd is
                    2.6e-3 from float64 here, so a kernel forming sigmoid(z) - bit misses the bound by 300 x)

Measured on an MI355X (``python -m pytest tests/test_gpu_train_cases.py -m gpu -s``); P positions, PC positions
per slab workgroup, e32 and the kernels' worst tensor against the float64 gradient, bound = 4 max(e32, 1e-6):

  case                         P   PC       e32     worst  worst / bound
  rt_slab64                 9072   64  1.31e-06  2.15e-06  0.409
  topo_a1_qpsk_u1            210   32  4.91e-07  3.86e-07  0.097
  topo_a3_noh_3heads_u5     1050   32  7.05e-07  5.49e-07  0.137
  topo_a4_noh_u2             420   32  5.08e-07  4.44e-07  0.111
  topo_a6_mask8_u16         3360   32  3.60e-07  1.80e-07  0.045
  topo_a8_64qam_u3           630   32  4.53e-07  4.46e-07  0.112
  topo_a9_b5_u7             1470   32  4.90e-07  3.07e-07  0.077
  topo_vario_a4              420   32  4.66e-07  4.16e-07  0.104
  grid_f1                     56   32  4.83e-07  5.58e-07  0.139
  grid_f2                    112   32  5.36e-07  5.21e-07  0.130
  grid_f13                   728   32  3.95e-07  3.15e-07  0.079
  dmrs_2                     280   32  4.69e-07  4.40e-07  0.110
  dmrs_2_3_10_11             280   32  4.54e-07  4.15e-07  0.104
  dmrs_0_13                  280   32  4.67e-07  4.55e-07  0.114
  dmrs_0_to_12               280   32  4.54e-07  4.34e-07  0.109
  bits_wide                  280   32  4.95e-07  4.51e-07  0.113
  none_mask_vario            420   32  5.37e-07  5.33e-07  0.133
  none_mask_masked           672   32  6.02e-07  4.72e-07  0.118
  dead_slots                 420   32  4.74e-07  4.63e-07  0.116
  confident                  280   32  3.30e-07  3.10e-07  0.077
"""
import numpy as np
import pytest
import torch

from tests import train_ref
from tests.memguard import Guarded, same_bits
from tests.test_gpu_train import check_adam_step, check_gradient_parity, on_device
from tests.test_train_ref import positions, trajectory_case

pytestmark = pytest.mark.gpu

K_MAX_SLABS = 256                    # kMaxSlabs of nrx_train.hip


def run_case(name):
    case, batch, sw, _ = train_ref.more_case(name)
    ref, ref32 = train_ref.more_references(name)
    P = positions(batch)
    PC = ((P + K_MAX_SLABS - 1) // K_MAX_SLABS + 31) // 32 * 32
    res = check_gradient_parity(name, case, batch, sw, ref, ref32, guarded=True)
    print(f"TABLE {name:26s} {P:5d} {PC:4d}  {res['e32']:.2e} {res['worst']:.2e}  {res['ratio']:.3f}")
    return case, batch, sw, ref, res, PC


def test_multi_step_slabs():
    case, batch, sw, ref, res, PC = run_case("rt_slab64")
    P = positions(batch)
    # two steps per workgroup and a tail in the last one, from the documented formula: a later change of
    # kMaxSlabs must not turn this back into a one-step case
    assert PC == 64 == train_ref.slab_positions(P) and P % PC == 48


@pytest.mark.parametrize("name", ["topo_" + n for n in train_ref.TOPO_NAMES])
def test_topology_sweep(name):
    run_case(name)


@pytest.mark.parametrize("name", ["grid_f1", "grid_f2", "grid_f13"])
def test_grid_edges(name):
    run_case(name)


@pytest.mark.parametrize("name", ["dmrs_2", "dmrs_2_3_10_11", "dmrs_0_13", "dmrs_0_to_12", "bits_wide"])
def test_loss_inputs(name):
    case, batch, sw, ref, res, _ = run_case(name)
    if name == "bits_wide":
        assert on_device(batch)[0].bits.shape[4] == 11 > case.spec.bits_max      # what becomes bits_stride


def test_mcs_mask_none_var_io():
    case, batch, sw, ref, res, _ = run_case("none_mask_vario")
    assert on_device(batch)[0].mcs_mask is None          # what Trainer._io gets
    n = len(res["grads"])
    for i in list(range(9, 18)) + list(range(n - 8, n - 4)):                     # StateInit 1, LLR head 1
        assert not res["grads"][i].any(), i
    assert all(res["grads"][i].any() for i in list(range(9)) + list(range(n - 12, n - 8)))


def test_mcs_mask_none_masked_head():
    case, batch, sw, ref, res, _ = run_case("none_mask_masked")
    assert on_device(batch)[0].mcs_mask is None
    nb = case.spec.bits[0]
    w2, b2 = res["grads"][-6], res["grads"][-5]
    assert not w2[:, nb:].any() and not b2[nb:].any() and w2[:, :nb].any() and b2[:nb].all()


def test_dead_slots_and_their_labels():
    """an all-zero slot and a slot without an active user: finite, the oracle's -- and the same bits whatever the
    labels of the slot nobody is active in"""
    from neural_rx_amd.train import Trainer
    case, batch, sw, ref, res, _ = run_case("dead_slots")
    alt = train_ref.more_case("dead_slots")[3]["alt"]
    runs = []
    for b in (batch, alt):
        sb, pe = on_device(b)
        tr = Trainer(case.spec, case.weights)
        tr.g.fill_(float("nan"))
        llr, h_ref = tr.grad_async(sb, pe, want_outputs=True, **sw)
        runs.append((tr.g.cpu().numpy(), tr.loss.cpu().numpy(), llr.cpu().numpy(), h_ref.cpu().numpy()))
    assert all(np.isfinite(a).all() for a in runs[0])
    for a, b in zip(*runs):
        assert same_bits(a, b)


def test_confident_and_correct():
    case, batch, sw, ref, res, _ = run_case("confident")
    z = ref["llr"][0]
    assert np.abs(z).min() >= 11.0                       # the small side of the sigmoid everywhere


def _state(tr):
    return [t.cpu().numpy() for t in (tr.w, tr.g, tr.m, tr.v, tr.loss)]


def test_side_stream_and_graph():
    """grad + Adam step on a side stream, then captured in a graph on it and replayed twice from the same w / m /
    v: w, g, m, v and the loss are the default stream's bits after one step.  The capture succeeding is the check
    that nothing in the call synchronises with the host."""
    from neural_rx_amd.train import Trainer
    case, batch = trajectory_case()
    sb, pe = on_device(batch)
    kw = dict(multiloss=True, w_chest=0.5)
    ref = Trainer(case.spec, case.weights)
    ref.grad_async(sb, pe, **kw)
    ref.step()
    torch.cuda.synchronize()
    want = _state(ref)
    tr = Trainer(case.spec, case.weights)
    w0 = tr.w.clone()
    assert all(np.isfinite(a).all() for a in want) and not same_bits(want[0], w0.cpu().numpy())
    io = tr._io(sb, pe, None, True, 0.5, (2, 11))
    ws = Guarded(tr.workspace_bytes(io), 0xFF)

    def reset():                                         # stream-ordered, on the current stream
        tr.w.copy_(w0)
        tr.m.zero_()
        tr.v.zero_()
        tr.g.fill_(float("nan"))
        tr.loss.fill_(float("nan"))
        ws.refill(0xFF)
        tr.num_steps = 0

    def one_step():
        tr.grad_async(sb, pe, workspace=ws.body, **kw)
        tr.step()

    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    got = {}
    with torch.cuda.stream(st):
        reset()
        one_step()
        st.synchronize()
        got["side stream"] = _state(tr)
        reset()
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            one_step()
        for tag in ("first replay", "second replay"):
            g.replay()
            got[tag] = _state(tr)
            reset()
        st.synchronize()
    ws.check("training workspace on the side stream")
    for tag, state in got.items():
        for what, a, b in zip("w g m v loss".split(), state, want):
            assert same_bits(a, b), (tag, what)


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("n", [1, 256 * 1024 + 1])
def test_adam_step_sizes(n, step):
    """one element, and one element past 1024 full workgroups"""
    check_adam_step(n, step)
