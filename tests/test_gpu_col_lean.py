"""The lean variants of the one-item column kernels (ColLean, csrc/nrx_geom.h; plan: tests/test_col_variants.py) at
the smallest shapes where their paths can go wrong, by the scheme of tests/test_gpu_col.py: the three-launch f16
forward with schedule mask 0 (strip kernels everywhere) against mask 29, ``np.array_equal`` on the raw LLRs and h_ref,
and the per-launch profile saying that the column kernels ran.

A handful of slots would go to the 8 / 16-row strip tiers, so the handle's small tiers are switched off
(``nrx_debug_small_tiers``, tests only) for both runs: mask 0 then runs the 24-row strip kernels, mask 29 the column
launches.

* nrx_rt, U = 2, F = 48, B = 3, one inactive user in one slot: lean, an odd batch; also against the fp64 oracle within
  the f16 gate of tests/test_gpu_parity.py
* nrx_rt, U = 1, F = 12, B = 2: positions 12..47 lie past the grid (clamped skip-row loads, row predication)
* the first shape without h_ref: the readout variant without the ChEst store
* the first shape without an MCS mask (the benchmark's call) and with a single-MCS mask that is not 1
* nrx_rt_var_mcs, U = 2, F = 48, B = 2, one-hot mask and no mask: the generic variant, the accumulating StateInit
* a 64-QAM masking model (bits_max = 6): the generic stores
"""
import ctypes
import dataclasses

import numpy as np
import pytest

from tests.helpers import compare, make_case, run_oracle

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _engine(case):
    from neural_rx_amd.receiver import CGNNEngine
    key = (case.spec, case.weights[0].tobytes()[:64], len(case.weights))
    if key not in _ENGINES:
        _ENGINES.clear()
        eng = CGNNEngine(case.spec, case.weights)
        fn = eng._lib.nrx_debug_small_tiers
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        assert fn(eng._h, 0) == 0
        eng.fused_config(enable=False)      # the three-launch forward (whose stages these are)
        _ENGINES[key] = eng
    return _ENGINES[key]


def _forward(case, sched, with_mask=True, want_h=True):
    import torch
    eng = _engine(case)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")
    eng.update_schedule(sched)
    eng.profile(True)
    llr, h = eng.forward(t(case.y), t(case.pe), t(case.h_hat), t(case.active),
                         t(case.mcs_mask) if with_mask else None, num_it=case.num_it, precision="f16", want_h=want_h)
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile(False)
    llr = llr.cpu().numpy()
    sp = case.spec
    out = {"llr": [llr[0 if sp.masking else m, ..., :nb] for m, nb in enumerate(sp.bits)], "llr_raw": llr,
           "h_hat": None if h is None else h.cpu().numpy()}
    return out, prof


def _check(case, n_col_updates=None, **kw):
    n_it = case.num_it or case.spec.num_it
    ref, pr = _forward(case, 0, **kw)
    got, pg = _forward(case, 29, **kw)
    assert pr["state_update_col"][0] == 0 and pr["state_init_col"][0] == 0 and pr["state_update"][0] == n_it, pr
    assert pr["state_init"][0] == 1, pr     # the 24-row tier's StateInit stage, not a small tier's
    assert pg["state_init_col"][0] == 1 and pg["state_init"][0] == 0, pg
    assert pg["state_update_col"][0] == (n_it if n_col_updates is None else n_col_updates), pg
    assert np.array_equal(ref["llr_raw"], got["llr_raw"]), np.abs(ref["llr_raw"] - got["llr_raw"]).max()
    if ref["h_hat"] is None:
        assert got["h_hat"] is None
    else:
        assert np.array_equal(ref["h_hat"], got["h_hat"])
    return ref, got


def _first_shape(**kw):
    active = np.ones((3, 2), np.float32)
    active[1, 0] = 0.0
    return make_case("nrx_rt", batch=3, users=2, prbs=4, snr_db=12, seed=171, active=active, **kw)


def test_lean_odd_batch_inactive_user_and_oracle():
    case = _first_shape()
    _, got = _check(case)
    assert np.isfinite(got["llr_raw"]).all() and np.abs(got["llr_raw"]).max() > 0
    c = compare(run_oracle(case), got)
    assert c["llr_rel"] < 0.10 and c["llr_rms_rel"] < 0.02 and c["flip_rate_confident"] <= 1e-3, c


def test_lean_rows_past_the_grid():
    _check(make_case("nrx_rt", batch=2, users=1, prbs=1, snr_db=12, seed=172))


def test_lean_readout_without_h_ref():
    case = _first_shape()
    with_h, _ = _forward(case, 29)
    ref, got = _check(case, want_h=False)
    assert got["h_hat"] is None
    # the LLRs do not depend on whether the ChEst head ran
    assert np.array_equal(with_h["llr_raw"], got["llr_raw"])


def test_lean_without_mask_and_with_a_single_mcs_weight():
    case = _first_shape()
    masked, _ = _forward(case, 29)
    _, plain = _check(case, with_mask=False)         # no mask: one-hot on MCS 0 = the mask of ones
    assert np.array_equal(masked["llr_raw"], plain["llr_raw"])
    # a single-MCS mask that is not 1 scales StateInit's output: the kernel's uniform branch
    w = np.full_like(case.mcs_mask, 0.5)
    w[0, 1] = 0.0
    _, scaled = _check(dataclasses.replace(case, mcs_mask=w))
    assert not np.array_equal(masked["llr_raw"], scaled["llr_raw"])


@pytest.mark.parametrize("with_mask", [True, False])
def test_generic_var_io_accumulates(with_mask):
    # two StateInit launches, the second adding onto the first; two LLR heads: the strip readout
    case = make_case("nrx_rt_var_mcs", batch=2, users=2, prbs=4, snr_db=14, seed=173,
                     mcs_choice=np.array([[0, 1], [1, 0]]))
    _check(case, n_col_updates=case.spec.num_it - 1, with_mask=with_mask)


def test_generic_64qam_masking_stores():
    # one StateInit, one 6-bit head (bits_max = 6): the per-element LLR stores of the generic readout
    case = make_case("nrx_large_var_mcs_64qam_masking", batch=2, users=2, prbs=4, snr_db=14, seed=174)
    _check(case)
