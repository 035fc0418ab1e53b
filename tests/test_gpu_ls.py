"""Cover-coded DMRS ports and the despreading LS estimator on the GPU (``nrx_ls_estimate``,
``nrx_generate_slots_dmrs``) against the numpy statement tests/dmrs_ref.py (needs an MI355X).

Tolerance of every float comparison with the reference: the generator's gate of tests/test_gpu_synth.py
and tests/test_gpu_cfo.py, 1e-6 relative to max |.| of the output plus 1e-7 absolute -- both sides
compute in f64 from the same f32 inputs and round once to f32.  Everything the library promises
bit-equal (repeat calls, batch splits, the generator against the estimator, the generator without a
``nrx_gen_dmrs`` against ``nrx_generate_slots_cfo``) is compared with ``array_equal``.

Separation (the property the feature exists for) is checked against the true channel: on a flat static
channel every element of ``h_hat - h`` lies within 6 sqrt(no / (2 n)) + 1e-6 max |h|, n = 4 the
despreading block -- six standard deviations of the despread LS noise (variance no / |p|^2 = no / 2
per pilot) plus the f32 rounding.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from oracle import synth_ref as S
from tests import dmrs_ref as D

pytestmark = pytest.mark.gpu


def _ports(numbers):
    from neural_rx_amd.ls import DMRSPorts
    return DMRSPorts.from_ports(numbers)


def _tuple(p):
    return list(p.cdm_group), list(p.focc), list(p.tocc)


def _close(a, b, name):
    scale = float(np.abs(b).max())
    err = float(np.abs(a.astype(np.float64) - b).max())
    print(f"{name}: max err {err:.3e}  scale {scale:.3e}")
    assert err <= 1e-6 * scale + 1e-7, (name, err, scale)


def _estimate(ports, y, pilots, active, dmrs, aerial):
    """nrx_ls_estimate on numpy inputs -> numpy (h_hat, h_ls_real, h_ls_imag or None)"""
    import torch
    from neural_rx_amd.ls import LSEstimator
    B, F, _, A2 = y.shape
    est = LSEstimator(ports, F, A2 // 2, dmrs, aerial=aerial)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = est(dev(y), dev(pilots), dev(active))
    torch.cuda.synchronize()
    out = out if aerial else (out, None, None)
    return tuple(None if o is None else o.cpu().numpy() for o in out)


# (F, A, port numbers, dmrs_symbols, B): one PRB and the scalar-store path; odd A; the time cover; F % 12 != 0
# (no Aerial list) with one symbol; several tiles and a tail; no cover and no despreading -- plain LS;
# then the wide kernels: k_ls_estimate<16> (A = 8); <32> (A = 16) where four DMRS symbols leave LDS room for
# 4 of the 8 ports per pass (57 600 bytes of dynamic LDS), so the port loop runs twice; and 7 ports on two
# tiles, the second of 8 subcarriers: passes of 4 + 3 ports, a partial tile in both.  An MI355X run: max error of
# h_hat 1.2e-7, 1.2e-7 and 6.0e-8 on these three (scale 1.4 to 1.8), of the Aerial lists 1.2e-7: one f32 ulp.
PARITY = [
    (12, 1, (0, 1, 2, 3), (2, 11), 3),
    (24, 3, (0, 1, 2, 3), (2, 11), 2),
    (24, 4, tuple(range(8)), (2, 3, 10, 11), 2),
    (8, 2, (0, 1), (2,), 1),
    (132, 4, (0, 1, 2, 3), (2, 11), 2),
    (12, 2, (0, 2), (2, 11), 1),
    (24, 8, (0, 1, 2, 3), (2, 11), 2),
    (24, 16, tuple(range(8)), (2, 3, 10, 11), 2),
    (40, 16, tuple(range(7)), (2, 3, 10, 11), 2),
]


@functools.lru_cache(maxsize=None)
def _inputs(F, A, numbers, dmrs, B):
    """(ports, y, pilots, active): normal y, the seeded base sequence (a table of arbitrary non-zero values
    for the plain-LS case), one inactive port per slot"""
    rng = np.random.default_rng(F * 100 + A)
    ports = _ports(numbers)
    y = rng.standard_normal((B, F, 14, 2 * A)).astype(np.float32)
    if ports.block == 1:
        pil = (rng.standard_normal((2, (F + 1) // 2, len(dmrs), 2)) + 3.0 * rng.choice([-1, 1], (2, 1, 1, 2))).astype(np.float32)
    else:
        pil = D.pilot_table(D.base_sequence(F + A, F, len(dmrs)))
    act = np.ones((B, len(numbers)), np.float32)
    for b in range(B):
        act[b, (b + 1) % len(numbers)] = 0.0
    return ports, y, pil, act


def _reference(ports, y, pil, act, dmrs):
    F = y.shape[1]
    h_ls, h_pair = D.ls_estimate(y, pil, dmrs, _tuple(ports), ports.despread_f, ports.despread_t, act)
    hh = D.h_hat(h_ls, _tuple(ports), F, dmrs)
    return (hh,) + (D.aerial_list(h_pair, F) if F % 12 == 0 else (None, None))


@pytest.mark.parametrize("F,A,numbers,dmrs,B", PARITY)
def test_estimator_matches_reference(F, A, numbers, dmrs, B):
    ports, y, pil, act = _inputs(F, A, numbers, dmrs, B)
    aerial = F % 12 == 0
    for active in (act, None):
        got = _estimate(ports, y, pil, active, dmrs, aerial)
        want = _reference(ports, y, pil, active, dmrs)
        for g, w, name in zip(got, want, ("h_hat", "h_ls_real", "h_ls_imag")):
            assert (g is None) == (w is None)
            if w is not None:
                assert g.shape == w.shape
                _close(g, w, name)
        if active is not None:      # inactive ports are exact zeros
            for b in range(B):
                u = (b + 1) % len(numbers)
                assert not got[0][b, u].any() and (not aerial or not got[1][b, :, u].any())
    # the covers do something: without despreading the estimate differs by more than the gate
    if ports.block > 1:
        assert np.abs(want[0] - D.h_hat(D.ls_estimate(y, pil, dmrs, _tuple(ports), False, False)[0], _tuple(ports), F,
                                        dmrs)).max() > 1e-2


@pytest.mark.parametrize("F,A,numbers,dmrs", [(132, 4, (0, 1, 2, 3), (2, 11)), (24, 4, tuple(range(8)), (2, 3, 10, 11)),
                                              (12, 1, (0, 1, 2, 3), (2, 11)), (24, 8, (0, 1, 2, 3), (2, 11)),
                                              (24, 16, tuple(range(8)), (2, 3, 10, 11))])
def test_repeat_calls_and_batch_splits_give_the_same_bits(F, A, numbers, dmrs):
    ports, y, pil, act = _inputs(F, A, numbers, dmrs, 4)
    whole = _estimate(ports, y, pil, act, dmrs, True)
    again = _estimate(ports, y, pil, act, dmrs, True)
    lo = _estimate(ports, y[:2], pil, act[:2], dmrs, True)
    hi = _estimate(ports, y[2:], pil, act[2:], dmrs, True)
    for w, a, l, h in zip(whole, again, lo, hi):
        np.testing.assert_array_equal(w, a)
        np.testing.assert_array_equal(w, np.concatenate([l, h]))


# ---------------------------------------------------------------- the generator
FIELDS = ("y", "h_hat", "h", "active", "mcs_mask", "mcs", "bits", "y_real", "y_imag", "h_ls_real", "h_ls_imag")


def _params(numbers, dmrs, cover=True, F=24, A=2, **kw):
    from neural_rx_amd.generator import GenParams
    ports = _ports(numbers)
    base = dict(num_tx=len(numbers), num_subcarriers=F, num_rx_ant=A, dmrs_symbols=dmrs, cdm_group=ports.cdm_group,
                mcs_bits=(2, 4), mcs_of_user=(-1,) + (1,) * (len(numbers) - 1), seed=77, dmrs=ports if cover else None)
    base.update(kw)
    return GenParams(**base)


def _host(sb):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in vars(sb).items() if v is not None}


@functools.lru_cache(maxsize=None)
def _generated(numbers, dmrs, cover, B=3, no=0.02, off=5):
    from neural_rx_amd.generator import SlotGenerator
    p = _params(numbers, dmrs, cover, num_active=len(numbers) - 1)
    return p, _host(SlotGenerator(p, want_h=True, aerial=True)(B, no, slot_offset=off))


def test_generator_without_dmrs_is_the_cfo_entry_point():
    """dmrs = NULL: every output bit-equal to nrx_generate_slots_cfo, the same workspace size"""
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.generator import SlotGenerator
    lib = _lib.load()
    p = _params((0, 2, 1, 3), (2, 11), cover=False, cdm_group=(0, 1, 0, 1), cfo_hz=300.0)
    gen = SlotGenerator(p, want_h=True, aerial=True)
    d = p.desc(3, 0.02, 5)
    n0, n1 = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.nrx_gen_workspace_size_cfo(ctypes.byref(d), ctypes.byref(gen._cfo), ctypes.byref(n0)) == 0
    assert lib.nrx_gen_workspace_size_dmrs(ctypes.byref(d), ctypes.byref(gen._cfo), None, ctypes.byref(n1)) == 0
    assert n0.value == n1.value
    outs = []
    for entry in ("cfo", "dmrs"):
        sb = gen._alloc(3)
        for k in FIELDS:
            getattr(sb, k).fill_(1 if k in ("mcs", "bits") else 7.0)
        ws = torch.full((n0.value,), 0xA5, dtype=torch.uint8, device="cuda")
        o = _lib.nrx_gen_out()
        for k in FIELDS:
            setattr(o, k, getattr(sb, k).data_ptr())
        o.bits_stride = p.bits_max
        gen._cfo.eps_out = sb.cfo_eps.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        if entry == "cfo":
            rc = lib.nrx_generate_slots_cfo(ctypes.byref(d), None, ctypes.byref(gen._cfo), ctypes.byref(o), ws.data_ptr(),
                                            ws.numel(), st)
        else:
            rc = lib.nrx_generate_slots_dmrs(ctypes.byref(d), None, ctypes.byref(gen._cfo), None, ctypes.byref(o),
                                             ws.data_ptr(), ws.numel(), st)
        assert rc == 0, lib.nrx_last_error()
        outs.append(_host(sb))
    for k in FIELDS + ("cfo_eps",):
        np.testing.assert_array_equal(outs[0][k], outs[1][k])
    assert np.abs(outs[0]["h_hat"]).max() > 0.1


@pytest.mark.parametrize("numbers,dmrs", [((0, 1, 2, 3), (2, 11)), (tuple(range(8)), (2, 3, 10, 11))])
def test_generator_with_cover_coded_ports(numbers, dmrs):
    p, g = _generated(numbers, dmrs, True)
    _, plain = _generated(numbers, dmrs, False)
    A, F, U = p.num_rx_ant, p.num_subcarriers, p.num_tx
    data = [t for t in range(14) if t not in dmrs]
    # what does not depend on the pilots keeps its bits
    for k in ("bits", "mcs", "mcs_mask", "active", "h"):
        np.testing.assert_array_equal(g[k], plain[k])
    np.testing.assert_array_equal(g["y"][:, :, data], plain["y"][:, :, data])
    assert np.abs(g["y"][:, :, list(dmrs)] - plain["y"][:, :, list(dmrs)]).max() > 1e-2
    np.testing.assert_array_equal(g["y_real"], g["y"][..., :A])
    np.testing.assert_array_equal(g["y_imag"], g["y"][..., A:])
    # the exported table is the seeded base sequence
    np.testing.assert_array_equal(g["pilots"], D.pilot_table(D.base_sequence(p.seed, F, len(dmrs))))
    # one definition: the generator's estimates are nrx_ls_estimate on its own y, table and active mask
    hh, hr, hi = _estimate(p.dmrs, g["y"], g["pilots"], g["active"], dmrs, True)
    np.testing.assert_array_equal(g["h_hat"], hh)
    np.testing.assert_array_equal(g["h_ls_real"], hr)
    np.testing.assert_array_equal(g["h_ls_imag"], hi)
    # y against the numpy statement (its y' is built on the f32 h: at most U 2^-25 2 sqrt(2) max |h| beyond
    # the two roundings the gate is made for, 6.7e-7 max |h| at U = 8 against a gate of 1e-6 max |y|)
    spec = S.GenSpec(batch=3, num_tx=U, num_subcarriers=F, num_rx_ant=A, dmrs_symbols=dmrs, cdm_group=p.cdm_group,
                     mcs_bits=p.mcs_bits, mcs_of_user=p.mcs_of_user, num_active=p.num_active, num_taps=p.num_taps,
                     num_sinusoids=p.num_sinusoids, max_delay_s=p.max_delay_s, max_doppler_hz=p.max_doppler_hz,
                     subcarrier_spacing=p.subcarrier_spacing, no=0.02, seed=p.seed, slot_offset=5)
    base, y_ref, x2, _ = D.generate(spec, _tuple(p.dmrs))
    np.testing.assert_array_equal(g["active"], base.active)
    np.testing.assert_array_equal(g["bits"], base.bits)
    _close(g["y"], y_ref, "y")
    _close(g["y"][:, :, list(dmrs)], y_ref[:, :, list(dmrs)], "y on the DMRS symbols")
    # ... and the estimates against the statement, from the generator's own y
    want = _reference(p.dmrs, g["y"], g["pilots"], g["active"], dmrs)
    for got, w, name in zip((g["h_hat"], g["h_ls_real"], g["h_ls_imag"]), want, ("h_hat", "h_ls_real", "h_ls_imag")):
        _close(got, w, name)


def test_cover_codes_separate_the_ports_of_a_group():
    """flat static channel, almost no noise, 8 active ports: the despread estimate is the true channel;
    today's generator (the same parameters without dmrs) leaves every port the sum of its group"""
    from neural_rx_amd.generator import SlotGenerator
    no, n = 1e-10, 4
    kw = dict(F=24, A=4, num_taps=1, max_delay_s=0.0, max_doppler_hz=0.0, mcs_of_user=(1,) * 8)
    err = {}
    for cover in (True, False):
        p = _params(tuple(range(8)), (2, 3, 10, 11), cover, **kw)
        g = _host(SlotGenerator(p, want_h=True)(4, no, slot_offset=11))
        assert g["active"].all()
        h = g["h"].astype(np.float64)
        err[cover] = g["h_hat"] - h
    bound = 6.0 * np.sqrt(no / (2 * n)) + 1e-6 * np.abs(h).max()
    rms = np.sqrt(np.mean(h ** 2) * 2)          # rms |h| of the complex channel
    print(f"max |h_hat - h| with cover {np.abs(err[True]).max():.3e} (bound {bound:.3e}); without, per port rms "
          f"{np.sqrt(np.mean(err[False] ** 2, axis=(0, 2, 3, 4)) * 2)} (rms |h| {rms:.3f})")
    assert np.abs(err[True]).max() <= bound
    for u in range(8):                          # every port shares its group with three others
        assert np.sqrt(np.mean(err[False][:, u] ** 2) * 2) > 0.1 * rms


def test_aerial_front_end_removes_the_frequency_cover():
    """nrx_aerial_preprocess on the generator's Aerial outputs under frequency cover: at every own pilot its
    h_hat is the generator's, within the gate (its pair average is f32 of f32-rounded inputs)"""
    import torch
    from tests.test_gpu_aerial_contract import engine
    p, g = _generated((0, 1, 2, 3), (2, 11), True)
    eng, _, _ = engine(num_rx_ant=p.num_rx_ant)
    U, dmrs = p.num_tx, p.dmrs_symbols
    ofdm = np.tile(np.array(dmrs, np.int32), (U, 1))
    scp = np.stack([np.arange(6, dtype=np.int32) * 2 + c for c in p.cdm_group])
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda()
         for a in (g["y_real"], g["y_imag"], g["h_ls_real"], g["h_ls_imag"], ofdm, scp)]
    y, h, _, _ = eng.aerial_preprocess(*t)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y.cpu().numpy(), g["y"])
    h = h.cpu().numpy()
    for u in range(U):
        f = np.arange(p.cdm_group[u], p.num_subcarriers, 2)
        _close(h[:, u][:, f][:, :, list(dmrs)], g["h_hat"][:, u][:, f][:, :, list(dmrs)], f"port {u} at its pilots")
    assert np.abs(g["h_hat"]).max() > 0.1


def test_evaluation_under_cover():
    """sim_ber_baseline with lsnn_lmmse and lmmse_lmmse on 4 cover-coded users: the run completes with finite
    counters on the data bits of the uncovered run (paired curves), and the refused combinations raise"""
    import torch
    from neural_rx_amd import chest
    from neural_rx_amd.baseline import BaselineReceiver
    from neural_rx_amd.cfo import CFOCompensator
    from neural_rx_amd.config import get_config
    from neural_rx_amd.evaluate import sim_ber_baseline
    from neural_rx_amd.generator import GenParams, SlotGenerator
    from neural_rx_amd.ls import DMRSPorts
    cfg = get_config("nrx_rt")
    ports = DMRSPorts.for_config(cfg, 4)
    assert ports.cdm_group == (0, 1, 0, 1) and ports.focc == (0, 0, 1, 1)        # ports 0, 2, 1, 3
    p = GenParams.from_config(cfg, num_tx=4, num_prbs=4, seed=9, dmrs=ports)
    plain = dataclasses.replace(p, dmrs=None)
    gen = SlotGenerator(p, want_h=True)
    cov = chest.estimate_covariance(gen, 32, 16).matrices()
    res = {}
    for system in ("baseline_lsnn_lmmse", "baseline_lmmse_lmmse"):
        rx = BaselineReceiver(system, p) if system in ("baseline_lsnn_lmmse",) else \
            chest.EstimatorBaselineReceiver(system, p, R_f=cov[0], R_t=cov[1])
        assert not rx.contaminated
        r = sim_ber_baseline(rx, gen, [8.0], batch_size=16, max_mc_iter=2, num_target_block_errors=10**9,
                             early_stop=False)
        assert r.mc_iters == [2] and r.slots == 32 and r.counts[0][1] > 0 and r.counts[0][3] == 32 * 4
        assert np.isfinite(r.ber[0]) and np.isfinite(r.bler[0]) and 0 <= r.ber[0] < 0.5
        res[system] = r
    print({k: (v.ber[0], v.bler[0]) for k, v in res.items()})
    # the despread estimates separate the users: today's lsnn_lmmse on the same slots is far worse
    r0 = sim_ber_baseline(BaselineReceiver("baseline_lsnn_lmmse", plain), SlotGenerator(plain, want_h=True), [8.0],
                          batch_size=16, max_mc_iter=2, num_target_block_errors=10**9, early_stop=False)
    assert r0.counts[0][1] == res["baseline_lsnn_lmmse"].counts[0][1]
    assert res["baseline_lsnn_lmmse"].counts[0][0] < r0.counts[0][0]
    a = gen(16, 0.1, slot_offset=3).bits.clone()
    b = SlotGenerator(plain)(16, 0.1, slot_offset=3).bits
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    # refused
    p8 = GenParams(num_tx=8, num_subcarriers=48, num_rx_ant=4, dmrs_symbols=(2, 3, 10, 11), dmrs=DMRSPorts.default(8))
    with pytest.raises(ValueError, match="3-D"):
        chest.ChannelEstimator("lmmse3", p)
    for kind in chest.KINDS:
        with pytest.raises(ValueError, match="time"):
            chest.ChannelEstimator(kind, p8)
    with pytest.raises(ValueError, match="time"):
        CFOCompensator(p8)
