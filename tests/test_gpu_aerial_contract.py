"""The Aerial / TensorRT contract of nrx_aerial.hip over the DMRS layouts, sizes and LLR heads it
accepts (needs an MI355X): k_aerial_tables, k_aerial_inputs, k_aerial_llr and k_llr_demap with
their host side in nrx_api.cpp and receiver.py.

* Preprocessing, observed directly through nrx_aerial_preprocess (the two launches
  nrx_forward_aerial runs, through the same helper), against oracle/pe_ref (pinned to a brute-force
  restatement over the same layout table by tests/test_aerial_layouts.py): nn, y and h_hat
  exactly -- the FOCC average is one f32 add and an exact halving on both sides -- and pe within
  one float32 ulp, exactly 0 where the oracle's is (both sides compute in f64 and round once; only
  the order of the variance sum differs).  Inputs are iid normal, so a gather from a neighbouring
  pilot pair is an O(1) error.  Sizes are chosen for the index arithmetic of k_aerial_inputs (its
  h_hat range of blocks starts at F T A rounded up to 256): F T A = 168 (less than one block), 1008
  (odd A, no multiple of 256), 10752 = 42 * 256 (an exact multiple), and U = 16.
* The whole forward on four seeded heads (single head, Var-IO without masking where bits[0] <
  bits_max and H > 1, masked, 64-QAM at A = 16 below the trained iteration count): equal, bit for
  bit, to the plain forward on the preprocessed tensors -- the same kernels on the same inputs at
  the same shape and precision -- and in f32x within the project's gates of the fp64 oracle run on
  the oracle-preprocessed case.
* The Python narrowing (inputs wider than U), the argument checks (return code and message, nothing
  launched) and nrx_llr_demap at its edges, the grid-stride loop past the 65536-block cap included.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

from neural_rx_amd import _lib
from neural_rx_amd import weights as W
from neural_rx_amd.config import get_config, spec_from_config
from oracle import pe_ref
from tests.helpers import Case, compare, run_oracle
from tests.test_aerial_layouts import LAYOUTS, aerial_inputs, layout_positions, within_one_ulp
from tests.test_gpu_parity import F32X_H_TOL, F32X_LLR_TOL
from tests.test_gpu_topologies import VARIO_A4, random_activity

pytestmark = pytest.mark.gpu

T = 14
# (B, F, A): F T A = 168 / 1008 / 10752
SIZES = {"one_prb_a1": (1, 12, 1), "odd_a3": (2, 24, 3), "mult256_a16": (3, 48, 16)}
PRE_CASES = [(name, "odd_a3", None) for name in LAYOUTS] + \
            [(name, size, None) for size in ("one_prb_a1", "mult256_a16")
             for name in ("type1_2sym", "three_sym_per_user")] + \
            [("type1_2sym", "odd_a3", 16)]

_ENGINES = {}


def engine(**spec_overrides):
    """One engine with seeded weights per topology."""
    from neural_rx_amd.receiver import CGNNEngine
    over = dict(dict(use_h_hat=True, bits=(4,), masking=False, num_it=2), **spec_overrides)
    spec = dataclasses.replace(spec_from_config(get_config("nrx_rt")), **over)
    if spec not in _ENGINES:
        weights = W.seeded(spec, 21)
        _ENGINES[spec] = (CGNNEngine(spec, weights), weights)
    return _ENGINES[spec][0], _ENGINES[spec][1], spec


def to_gpu(inputs):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inputs.items()}


FEED = ("y_real", "y_imag", "h_ls_real", "h_ls_imag", "dmrs_ofdm_pos", "dmrs_subcarrier_pos")


def oracle_preprocess(x, U):
    y, h, pe = pe_ref.aerial_preprocess(x["y_real"], x["y_imag"], x["h_ls_real"], x["h_ls_imag"],
                                        x["dmrs_ofdm_pos"], x["dmrs_subcarrier_pos"], U)
    nn, _ = pe_ref.aerial_nn_indices(x["dmrs_ofdm_pos"], x["dmrs_subcarrier_pos"], T, y.shape[1] // 12)
    return y, h, pe, nn[:, 0]


# ---------------------------------------------------------------- preprocessing
@pytest.mark.parametrize("name,size,users", PRE_CASES, ids=[f"{n}-{s}-u{u or len(LAYOUTS[n][0])}"
                                                            for n, s, u in PRE_CASES])
def test_preprocess_matches_oracle(name, size, users):
    import torch
    B, F, A = SIZES[size]
    eng, _, _ = engine(num_rx_ant=A)
    x = aerial_inputs(name, B, F, A, seed=31, users=users)
    U = x["dmrs_ofdm_pos"].shape[0]
    t = to_gpu(x)
    y, h, pe, nn = eng.aerial_preprocess(*[t[k] for k in FEED])
    torch.cuda.synchronize()
    assert tuple(y.shape) == (B, F, T, 2 * A) and tuple(h.shape) == (B, U, F, T, 2 * A)
    assert tuple(pe.shape) == (U, F, T, 2) and tuple(nn.shape) == (U, T, 12) and nn.dtype == torch.int32
    ry, rh, rpe, rnn = oracle_preprocess(x, U)
    np.testing.assert_array_equal(nn.cpu().numpy(), rnn)
    np.testing.assert_array_equal(y.cpu().numpy(), ry)
    np.testing.assert_array_equal(h.cpu().numpy(), rh)
    got = pe.cpu().numpy()
    print(f"PE {name} {size}: max|d| {np.abs(got - rpe).max():.3e}, differing {int((got != rpe).sum())}")
    assert within_one_ulp(got, rpe), np.abs(got - rpe).max()
    if name == "all_pilots":
        assert not got.any()
    if name == "all_sc_one_sym":
        assert not got[..., 1].any()


# ---------------------------------------------------------------- the whole forward
HEADS = {
    "single_head": dict(spec=dict(num_rx_ant=4), users=2, layout="type1_2sym"),
    "vario_unmasked": dict(spec=VARIO_A4["spec"], users=2, layout="three_sym_per_user"),
    "masked": dict(spec=dict(num_rx_ant=3, bits=(2, 4, 6), masking=True), users=3, layout="type2_npil4"),
    "qam64_a16": dict(spec=dict(num_rx_ant=16, bits=(6,), num_it=3), users=4, layout="one_sym_u3", run_it=2),
}
_FWD = {}


def forward_case(head):
    """(engine, weights, spec, feed dict, activity [3, U], num_it) of one head at F = 24, B = 3."""
    if head not in _FWD:
        hd = HEADS[head]
        eng, weights, spec = engine(**hd["spec"])
        k = list(HEADS).index(head)
        x = aerial_inputs(hd["layout"], 3, 24, spec.num_rx_ant, seed=41 + k, users=hd["users"])
        act = random_activity(np.random.default_rng(5 + k), 3, hd["users"])
        assert (act == 0).any()
        _FWD[head] = (eng, weights, spec, x, act, hd.get("run_it"))
    return _FWD[head]


def run_aerial(eng, t, act, num_it, prec, want_h=True):
    import torch
    llr, h = eng.forward_aerial(t["y_real"], t["y_imag"], t["h_ls_real"], t["h_ls_imag"], act,
                                t["dmrs_ofdm_pos"], t["dmrs_subcarrier_pos"], num_it=num_it, precision=prec,
                                want_h=want_h)
    torch.cuda.synchronize()
    return llr, h


@pytest.mark.parametrize("prec", ["f32x", "f16"])
@pytest.mark.parametrize("head", list(HEADS))
def test_aerial_forward_equals_plain_forward(head, prec):
    import torch
    eng, _, spec, x, act, num_it = forward_case(head)
    U = act.shape[1]
    bits0 = spec.bits_max if spec.masking else spec.bits[0]
    t = to_gpu(x)
    act_t = torch.from_numpy(act).cuda()
    llr_a, h_a = run_aerial(eng, t, act_t, num_it, prec)
    assert tuple(llr_a.shape) == (3, bits0, U, 24, T)
    y, h, pe, _ = eng.aerial_preprocess(*[t[k] for k in FEED])
    raw, h_p = eng.forward(y, pe, h, act_t, None, num_it=num_it, precision=prec)
    torch.cuda.synchronize()
    assert tuple(raw.shape) == (spec.num_llr_heads, 3, U, 24, T, spec.bits_max)
    assert torch.isfinite(llr_a).all() and torch.isfinite(h_a).all()
    assert torch.equal(llr_a, -raw[0][..., :bits0].permute(0, 4, 1, 2, 3))
    assert torch.equal(h_a, h_p)
    llr_n, h_n = run_aerial(eng, t, act_t, num_it, prec, want_h=False)
    assert h_n is None and torch.equal(llr_n, llr_a)


@pytest.mark.parametrize("head", list(HEADS))
def test_aerial_forward_matches_oracle_f32x(head):
    import torch
    eng, weights, spec, x, act, num_it = forward_case(head)
    U = act.shape[1]
    y, h, pe, _ = oracle_preprocess(x, U)
    mask = np.zeros((3, U, spec.num_mcs), np.float32)
    mask[..., 0] = 1.0
    ref = run_oracle(Case(head, None, spec, weights, y, pe, h, act, mask, None, num_it))
    # a masked model has one head of bits_max LLRs (its per-MCS outputs are slices of it)
    ref_llr = ref["llr"][spec.bits.index(spec.bits_max)] if spec.masking else ref["llr"][0]
    llr_a, h_a = run_aerial(eng, to_gpu(x), torch.from_numpy(act).cuda(), num_it, "f32x")
    got = {"llr": [-np.transpose(llr_a.cpu().numpy(), (0, 2, 3, 4, 1))], "h_hat": h_a.cpu().numpy()}
    assert got["llr"][0].shape == ref_llr.shape
    c = compare({"llr": [ref_llr], "h_hat": ref["h_hat"]}, got)
    print(f"AERIAL f32x {head}: llr max-abs {c['llr_maxabs']:.3e} (max |LLR| {c['llr_max']:.2f}), "
          f"h max-abs {c['h_maxabs']:.3e}")
    assert c["llr_maxabs"] < F32X_LLR_TOL, c
    assert c["h_maxabs"] < F32X_H_TOL, c


# ---------------------------------------------------------------- narrowing
def test_inputs_wider_than_num_tx_are_narrowed():
    # h_ls with four user columns, positions with four rows, dmrs_port_mask with four columns, U = 2:
    # the surplus is NaN / another pattern and must not be read
    import torch
    from neural_rx_amd.receiver import AerialReceiver
    cfg = get_config("nrx_rt")
    spec = spec_from_config(cfg)
    B, F, A = 2, 24, spec.num_rx_ant
    x = aerial_inputs("type1_2sym", B, F, A, seed=53)
    wide = dict(x)
    for k in ("h_ls_real", "h_ls_imag"):
        wide[k] = np.concatenate([x[k], np.full_like(x[k], np.nan)], axis=2)
    wide["dmrs_ofdm_pos"] = np.concatenate([x["dmrs_ofdm_pos"], np.array([[13, 0], [5, 6]], np.int32)])
    wide["dmrs_subcarrier_pos"] = np.concatenate([x["dmrs_subcarrier_pos"],
                                                  np.array([[11, 9, 7, 5, 3, 1], [0, 1, 2, 3, 4, 5]], np.int32)])
    act = np.array([[1, 0], [1, 1]], np.float32)
    act_wide = np.concatenate([act, np.ones_like(act)], axis=1)
    t, tw = to_gpu(x), to_gpu(wide)
    act_t, act_w = torch.from_numpy(act).cuda(), torch.from_numpy(act_wide).cuda()
    for prec in ("f32x", "f16"):
        nrx = AerialReceiver(cfg, weight_list=W.seeded(spec, 21), precision=prec, num_tx=2)
        want_llr, want_h = run_aerial(nrx.engine, t, act_t, nrx.num_it, prec)
        assert torch.isfinite(want_llr).all()
        llr, h = nrx((tw["y_real"], tw["y_imag"], tw["h_ls_real"], tw["h_ls_imag"], act_w, tw["dmrs_ofdm_pos"],
                      tw["dmrs_subcarrier_pos"]))
        torch.cuda.synchronize()
        assert tuple(llr.shape) == (B, 4, 2, F, T)
        assert torch.equal(llr, want_llr) and torch.equal(h, want_h)
        # forward_aerial itself: U from the mask it is given, here a non-contiguous view
        llr, h = run_aerial(nrx.engine, tw, act_w[:, :2], nrx.num_it, prec)
        assert torch.equal(llr, want_llr) and torch.equal(h, want_h)
    want = nrx.engine.aerial_preprocess(*[t[k] for k in FEED])
    got = nrx.engine.aerial_preprocess(*[tw[k] for k in FEED], num_tx=2)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.equal(g, w)


# ---------------------------------------------------------------- argument checks
def test_argument_checks_reject_before_any_launch():
    import torch
    eng, _, spec = engine(num_rx_ant=4)
    lib = eng._lib
    B, F, U, A = 2, 24, 2, 4
    t = to_gpu(aerial_inputs("type1_2sym", B, F, A, seed=61))
    act = torch.ones((B, U), dtype=torch.float32, device="cuda")
    llr = torch.empty((B, 4, U, F, T), dtype=torch.float32, device="cuda")
    outs = eng.aerial_preprocess(*[t[k] for k in FEED])          # buffers of the right sizes
    torch.cuda.synchronize()

    def good():
        io, _ = eng._aerial_io(*[t[k] for k in FEED], U)
        io.num_it, io.precision = spec.num_it, _lib.NRX_PREC_F32X
        io.dmrs_port_mask, io.llr = act.data_ptr(), llr.data_ptr()
        return io

    need = ctypes.c_size_t()
    assert lib.nrx_aerial_workspace_size(eng._h, ctypes.byref(good()), ctypes.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")

    def calls(io, pre_args=None):
        p = [o.data_ptr() for o in outs] if pre_args is None else pre_args
        return {"forward": lambda: lib.nrx_forward_aerial(eng._h, ctypes.byref(io), ws.data_ptr(), ws.numel(), None),
                "size": lambda: lib.nrx_aerial_workspace_size(eng._h, ctypes.byref(io), ctypes.byref(need)),
                "pre": lambda: lib.nrx_aerial_preprocess(eng._h, ctypes.byref(io), *p, None)}

    def rejected(fn, code, text):
        rc = fn()
        msg = lib.nrx_last_error().decode()
        assert rc == code and text in msg, (rc, msg)

    SHAPE, ARG, WORKSPACE = -2, _lib.NRX_ERR_INVALID_ARG, _lib.NRX_ERR_WORKSPACE
    shape_cases = [("num_subcarriers", 20, "multiple of 12")] + \
                  [("num_dmrs_subcarriers", v, "num_dmrs_subcarriers must be even and 2..12") for v in (3, 0, 14)] + \
                  [("num_dmrs_symbols", v, "num_dmrs_symbols must be 1..14") for v in (0, 15)]
    for field, value, text in shape_cases:
        io = good()
        setattr(io.shape if field == "num_subcarriers" else io, field, value)
        for fn in calls(io).values():
            rejected(fn, SHAPE, text)
    io = good()
    io.llr = None
    rejected(calls(io)["forward"], ARG, "null tensor pointer")
    io = good()
    rejected(lambda: lib.nrx_forward_aerial(eng._h, ctypes.byref(io), ws.data_ptr(), need.value - 1, None),
             WORKSPACE, f"workspace too small: need {need.value} bytes")
    rejected(lambda: lib.nrx_forward_aerial(eng._h, ctypes.byref(io), None, need.value, None),
             WORKSPACE, "workspace too small")
    # the new entry point's own checks: it needs neither llr nor dmrs_port_mask ...
    io = good()
    io.llr = io.dmrs_port_mask = io.h_hat = None
    assert calls(io)["pre"]() == 0
    # ... but every input it reads and every output it writes
    for field in FEED:
        io = good()
        setattr(io, field, None)
        rejected(calls(io)["pre"], ARG, "null tensor pointer")
    for k in range(4):
        p = [o.data_ptr() for o in outs]
        p[k] = None
        rejected(calls(good(), p)["pre"], ARG, "null output pointer")
    p = [o.data_ptr() for o in outs]
    rejected(lambda: lib.nrx_aerial_preprocess(None, ctypes.byref(good()), *p, None), ARG, "null argument")
    rejected(lambda: lib.nrx_aerial_preprocess(eng._h, None, *p, None), ARG, "null argument")
    torch.cuda.synchronize()
    # the rejected calls wrote nothing
    for o, w in zip(eng.aerial_preprocess(*[t[k] for k in FEED]), outs):
        assert torch.equal(o, w)


# ---------------------------------------------------------------- nrx_llr_demap
def _subset(F, n_sym):
    rng = np.random.default_rng(71)
    return rng.permutation(F * n_sym)[:101]


DEMAP_CASES = {
    # (B, U, F, T, stride, bits, RE table: None = all REs in grid order)
    "bits_eq_stride_f13": (2, 3, 13, 14, 4, 4, None),
    "one_re_last": (1, 1, 12, 14, 8, 1, np.array([12 * 14 - 1])),
    "unsorted_subset": (2, 2, 24, 14, 6, 3, _subset(24, 14)),
    "t5": (3, 2, 12, 5, 2, 2, None),
    # 17.2 M outputs > 65536 blocks x 256 threads: the grid-stride loop takes a second trip
    "past_block_cap": (64, 16, 150, 14, 8, 8, None),
}


@pytest.mark.parametrize("name", list(DEMAP_CASES))
def test_llr_demap_edges(name):
    import torch
    B, U, F, Tn, stride, bits, re = DEMAP_CASES[name]
    re = np.arange(F * Tn) if re is None else np.asarray(re)
    n = B * U * F * Tn * stride
    if name == "past_block_cap":
        assert B * U * re.size * bits > 65536 * 256
    if name == "unsorted_subset":
        assert (np.diff(re) < 0).any() and np.unique(re).size == re.size
    # every LLR encodes its own flat index (modulo 2^24, where float32 stops being exact)
    llr = (np.arange(n, dtype=np.int64) % (1 << 24)).astype(np.float32).reshape(B, U, F, Tn, stride)
    eng, _, _ = engine(num_rx_ant=4)
    out = eng.llr_demap(torch.from_numpy(llr).cuda(), bits, torch.from_numpy(re.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    t, f = re // F, re % F
    want = llr[:, :, f, t, :bits].reshape(B, U, re.size * bits)
    got = out.cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)
