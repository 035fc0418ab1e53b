"""The carrier frequency offset on the GPU (``nrx_generate_slots_cfo``, ``nrx_cfo_estimate``,
``nrx_cfo_rotate``) against the numpy statement tests/cfo_ref.py (needs an MI355X).

Tolerances: float outputs (y, h_hat, h, the Aerial outputs, the rotated estimates) within the
generator's bound of tests/test_gpu_synth.py, 1e-6 relative to max |.| plus 1e-7 absolute: both sides
compute in f64 and round once to f32 (h under ``h_with_phase`` twice, 2^-23 at the most; the
reference's y' uses the f32 h, 2^-24 |h| |x' - x|).  eps: 1e-12 absolute and the bits.  eps_hat: 1e-9
absolute (both sides sum the same f64 products, in another order).

Properties (static channel, F = 24, A = 2, U = 2, B = 32, no = 1e-3), each asserted for the numpy
reference first and then for the GPU:
* estimator, |eps| <= 0.04: max |eps_hat - eps| over the active users < 2e-3;
* compensation, |eps| <= 0.03, ``h_with_phase``: the NMSE of the compensated nearest-neighbour h_hat
  is at most 1/4 of the uncompensated one.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from oracle import synth_ref as S
from tests import cfo_ref as R
from tests import synth_chan_ref as C

pytestmark = pytest.mark.gpu

FIELDS = ("y", "h_hat", "h", "active", "mcs_mask", "mcs", "bits")


def _params(F, **kw):
    from neural_rx_amd.generator import GenParams
    base = dict(num_tx=2, num_subcarriers=F, num_rx_ant=2, cdm_group=(0, 1), mcs_bits=(2, 4), mcs_of_user=(-1, 1),
                seed=31)
    base.update(kw)
    return GenParams(**base)


def _spec(p, batch, no, off=0):
    return S.GenSpec(batch=batch, num_tx=p.num_tx, num_subcarriers=p.num_subcarriers, num_rx_ant=p.num_rx_ant,
                     dmrs_symbols=p.dmrs_symbols, cdm_group=p.cdm_group, mcs_bits=p.mcs_bits,
                     mcs_of_user=p.mcs_of_user, num_active=p.num_active, num_taps=p.num_taps,
                     num_sinusoids=p.num_sinusoids, max_delay_s=p.max_delay_s, max_doppler_hz=p.max_doppler_hz,
                     subcarrier_spacing=p.subcarrier_spacing, no=no, seed=p.seed, slot_offset=off)


def _ref(p, batch, no, off=0):
    s = _spec(p, batch, no, off)
    base = C.generate(s, p.profiles(), p.rx_mix()) if p.correlated else None
    return R.generate(s, p.cfo_per_port(), p.cfo_constant, p.fft_size, p.h_with_phase, base=base)


def _host(sb):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in vars(sb).items() if v is not None}


def _gpu(p, batch, no, off=0, aerial=False):
    from neural_rx_amd.generator import SlotGenerator
    return _host(SlotGenerator(p, want_h=True, aerial=aerial)(batch, no, slot_offset=off))


def _close(a, b, name):
    scale = float(np.abs(b).max())
    err = float(np.abs(a.astype(np.float64) - b).max())
    assert err <= 1e-6 * scale + 1e-7, (name, err, scale)


# F = 24, N = F: the circulant wrap; F = 36, N = 64: no multiple of 16, and an offset beyond one spacing;
# F = 2: the generator's minimum; F = 132: three output tiles and five K chunks
PARITY = [
    (24, 0, False, 2, False, (900.0, 2400.0)), (24, 0, True, 1, True, (900.0, 2400.0)),
    (36, 64, False, 1, True, (1500.0, 300.0)), (36, 64, True, 2, False, (36e3, 400.0)),
    (2, 0, False, 2, True, (900.0, 2400.0)), (2, 16, True, 1, False, (900.0, 2400.0)),
    (132, 0, False, 2, False, (2400.0, 900.0)), (132, 256, True, 1, True, (0.0, 15e3)),
]


def _parity(p, B=3, no=0.02, off=7):
    aerial = p.num_subcarriers % 12 == 0
    g = _gpu(p, B, no, off, aerial=aerial)
    o = _ref(p, B, no, off)
    for k in ("active", "mcs", "bits"):
        np.testing.assert_array_equal(g[k], getattr(o.base, k))
    assert np.abs(g["cfo_eps"] - o.eps).max() <= 1e-12
    np.testing.assert_array_equal(g["cfo_eps"], o.eps)
    _close(g["y"], o.y, "y")
    _close(g["h_hat"], o.h_hat, "h_hat")
    _close(g["h"], o.h, "h")
    if aerial:
        A = p.num_rx_ant
        _close(g["y_real"], o.y[..., :A], "y_real")
        _close(g["y_imag"], o.y[..., A:], "y_imag")
        hr, hi = R.aerial_pilots(o.h_hat, p.dmrs_symbols, p.cdm_group)
        _close(g["h_ls_real"], hr, "h_ls_real")
        _close(g["h_ls_imag"], hi, "h_ls_imag")
    # the offset is there: y differs from the generator without it by more than the gate
    assert np.abs(o.y - o.base.y).max() > 1e-3
    return g, o


@pytest.mark.parametrize("F,N,constant,active,phase,hz", PARITY)
def test_generator_matches_reference(F, N, constant, active, phase, hz):
    p = _params(F, cfo_hz=hz, cfo_constant=constant, fft_size=N, h_with_phase=phase, num_active=active)
    g, o = _parity(p)
    if phase:
        assert np.abs(o.h - o.base.h).max() > 1e-3
    else:
        np.testing.assert_array_equal(g["h"], _gpu(dataclasses.replace(p, cfo_hz=None), 3, 0.02, 7)["h"])


def test_generator_matches_reference_on_a_correlated_channel():
    from neural_rx_amd.generator import rx_correlation
    p = _params(24, cfo_hz=(1200.0, 600.0), fft_size=32, h_with_phase=True,
                user_profiles=[(100e-9, 400.0), (600e-9, 50.0)], rx_corr=rx_correlation(2, 0.7))
    _parity(p)


def _raw(p, batch, no, cfo, entry="cfo", off=3):
    """nrx_generate_slots_cfo with a given nrx_gen_cfo / None, or nrx_generate_slots_ex, in a workspace
    of exactly the size its *_workspace_size call asks for; (outputs, workspace bytes)"""
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.generator import SlotGenerator
    lib = _lib.load()
    g = SlotGenerator(dataclasses.replace(p, cfo_hz=None), want_h=True)
    sb = g._alloc(batch)
    d = p.desc(batch, no, off)
    o = _lib.nrx_gen_out()
    o.y, o.h_hat, o.h, o.active = (t.data_ptr() for t in (sb.y, sb.h_hat, sb.h, sb.active))
    o.mcs_mask, o.mcs, o.bits, o.bits_stride = sb.mcs_mask.data_ptr(), sb.mcs.data_ptr(), sb.bits.data_ptr(), p.bits_max
    n = ctypes.c_size_t()
    st = torch.cuda.current_stream().cuda_stream
    if entry == "ex":
        _lib.check(lib.nrx_gen_workspace_size(ctypes.byref(d), ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        _lib.check(lib.nrx_generate_slots_ex(ctypes.byref(d), None, ctypes.byref(o), ws.data_ptr(), ws.numel(), st))
    else:
        c = ctypes.byref(cfo) if cfo is not None else None
        _lib.check(lib.nrx_gen_workspace_size_cfo(ctypes.byref(d), c, ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        _lib.check(lib.nrx_generate_slots_cfo(ctypes.byref(d), None, c, ctypes.byref(o), ws.data_ptr(), ws.numel(), st))
    torch.cuda.synchronize()
    return {k: getattr(sb, k).cpu().numpy().copy() for k in FIELDS}, n.value


def test_no_offset_is_bit_identical_to_generate_slots_ex():
    import torch
    from neural_rx_amd import _lib
    p = _params(36)
    old, size = _raw(p, 3, 0.05, None, entry="ex")
    null, size_null = _raw(p, 3, 0.05, None)
    zero = _lib.nrx_gen_cfo()
    zero.cfo_hz[2] = 500.0                     # a port >= U: not read
    zero.h_with_phase, zero.constant, zero.fft_size = 1, 1, 64
    eps = torch.full((3, 2), 7.0, dtype=torch.float64, device="cuda")
    zero.eps_out = eps.data_ptr()
    zeros, size_zero = _raw(p, 3, 0.05, zero)
    assert size_null == size and size_zero == size
    for k in FIELDS:
        np.testing.assert_array_equal(null[k], old[k], err_msg=k)
        np.testing.assert_array_equal(zeros[k], old[k], err_msg=k)
    assert (eps.cpu().numpy() == 7.0).all()        # nothing new was launched
    on = _lib.nrx_gen_cfo()
    on.cfo_hz[1] = 500.0
    changed, size_on = _raw(p, 3, 0.05, on)
    assert size_on == size + (3 * 2 * 36 * 14 * 16 + 255) // 256 * 256
    assert np.abs(changed["y"] - old["y"]).max() > 1e-3
    np.testing.assert_array_equal(changed["bits"], old["bits"])


def test_split_invariance_and_repeatability():
    p = _params(36, cfo_hz=(900.0, 2400.0), fft_size=64, h_with_phase=True, num_active=1)
    keys = ("y", "h_hat", "h", "cfo_eps", "active", "bits")
    full = _gpu(p, 6, 0.05)
    again = _gpu(p, 6, 0.05)
    first, second = _gpu(p, 3, 0.05), _gpu(p, 3, 0.05, off=3)
    for k in keys:
        np.testing.assert_array_equal(again[k], full[k], err_msg=k)
        np.testing.assert_array_equal(first[k], full[k][:3], err_msg=k)
        np.testing.assert_array_equal(second[k], full[k][3:], err_msg=k)


def _comp_gpu(p, g):
    """(eps_hat, h_hat rotated NEAREST_DMRS +1 out of place, h_hat rotated ZERO -1 in place) on the GPU"""
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.cfo import CFOCompensator
    from neural_rx_amd.generator import SlotBatch
    comp = CFOCompensator(p)
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    sb = SlotBatch(y=None, h_hat=t(g["h_hat"]), active=t(g["active"]), mcs_mask=None, mcs=None, bits=None)
    eps = comp.estimate(sb)
    nn = comp.apply_nn(sb, eps=eps).h_hat
    assert nn.data_ptr() != sb.h_hat.data_ptr()
    np.testing.assert_array_equal(sb.h_hat.cpu().numpy(), g["h_hat"])      # apply_nn leaves the batch alone
    flat = comp.rotate(sb.h_hat.clone(), eps, _lib.CFO_REF_ZERO, -1)
    torch.cuda.synchronize()
    return eps.cpu().numpy(), nn.cpu().numpy(), flat.cpu().numpy()


@pytest.mark.parametrize("dmrs", [(2, 11), (2, 7, 11), (3,)])
def test_estimate_and_rotate_match_reference(dmrs):
    p = _params(26, num_rx_ant=3, dmrs_symbols=dmrs, cfo_hz=(900.0, 1200.0), num_active=1, cdm_group=(1, 0))
    g = _gpu(p, 5, 0.01)
    eps, nn, flat = _comp_gpu(p, g)
    ref = R.estimate(g["h_hat"], g["active"], dmrs, p.cdm_group)
    assert np.abs(eps - ref).max() <= 1e-9
    assert (eps[g["active"] <= 0] == 0).all()
    if len(dmrs) < 2:
        assert (eps == 0).all()
        eps = np.broadcast_to(np.array([0.02, -0.03]), eps.shape).copy()   # still rotate by something
        import torch
        from neural_rx_amd import _lib
        from neural_rx_amd.cfo import CFOCompensator
        comp, e = CFOCompensator(p), torch.from_numpy(eps).cuda()
        nn = comp.rotate(torch.from_numpy(g["h_hat"]).cuda(), e, _lib.CFO_REF_NEAREST_DMRS, +1).cpu().numpy()
        flat = comp.rotate(torch.from_numpy(g["h_hat"]).cuda(), e, _lib.CFO_REF_ZERO, -1).cpu().numpy()
    else:
        assert np.abs(eps[g["active"] > 0]).min() > 1e-4
    _close(nn, R.rotate(g["h_hat"], eps, dmrs, R.REF_NEAREST_DMRS, +1), "nearest")
    _close(flat, R.rotate(g["h_hat"], eps, dmrs, R.REF_ZERO, -1), "zero")


@functools.lru_cache(maxsize=None)
def _static(max_hz, phase):
    """(params, GPU outputs, reference) of the property setup"""
    p = _params(24, cfo_hz=max_hz, h_with_phase=phase, max_doppler_hz=0.0, mcs_of_user=(0, 1), seed=77)
    return p, _gpu(p, 32, 1e-3), _ref(p, 32, 1e-3)


def test_estimator_recovers_the_offset():
    p, g, o = _static(1200.0, False)
    act = o.base.active > 0
    assert 0.02 < np.abs(o.eps).max() <= 0.04
    ref = R.estimate(o.h_hat, o.base.active, p.dmrs_symbols, p.cdm_group)
    worst = np.abs(ref - o.eps)[act].max()
    print("reference max |eps_hat - eps|:", worst)
    assert worst < 2e-3
    eps, _, _ = _comp_gpu(p, g)
    print("gpu max |eps_hat - eps|:", np.abs(eps - g["cfo_eps"])[act].max())
    assert np.abs(eps - R.estimate(g["h_hat"], g["active"], p.dmrs_symbols, p.cdm_group)).max() <= 1e-9
    assert np.abs(eps - ref).max() <= 1e-6        # the two h_hat differ by f32 ulps
    assert np.abs(eps - g["cfo_eps"])[act].max() < 2e-3


def test_compensation_cuts_the_nmse():
    import torch
    from neural_rx_amd.softmetrics import SoftAccumulator
    p, g, o = _static(900.0, True)
    ref_eps = R.estimate(o.h_hat, o.base.active, p.dmrs_symbols, p.cdm_group)
    ref_nn = R.rotate(o.h_hat, ref_eps, p.dmrs_symbols, R.REF_NEAREST_DMRS, +1)
    r0, r1 = R.nmse(o.h_hat, o.h, o.base.active), R.nmse(ref_nn, o.h, o.base.active)
    print("reference NMSE uncompensated / compensated:", r0, r1)
    assert r1 <= 0.25 * r0
    _, nn, _ = _comp_gpu(p, g)

    def gpu_nmse(h_est):
        acc = SoftAccumulator(p.num_tx, p.mcs_bits)
        acc.add_channel(torch.from_numpy(h_est).cuda(), torch.from_numpy(g["h"]).cuda(), torch.from_numpy(g["active"]).cuda())
        torch.cuda.synchronize()
        a = acc.arrays()
        return float(a["err"].sum() / a["ref"].sum())

    g0, g1 = gpu_nmse(g["h_hat"]), gpu_nmse(nn)
    print("gpu NMSE uncompensated / compensated:", g0, g1)
    assert g1 <= 0.25 * g0
    assert abs(g0 - r0) <= 1e-4 * r0 and abs(g1 - r1) <= 1e-3 * r1


def test_wrapped_estimator_removes_the_rotation_from_the_interpolation():
    """ChannelEstimator(cfo=...) equals de-rotate, estimate, re-rotate by hand, bit for bit, and the
    linear interpolation gains from it under an offset"""
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.cfo import CFOCompensator
    from neural_rx_amd.chest import ChannelEstimator
    from neural_rx_amd.generator import SlotGenerator
    p, g, o = _static(900.0, True)
    sb = SlotGenerator(p, want_h=True)(32, 1e-3)
    comp = CFOCompensator(p)
    plain = ChannelEstimator("lin", p)(sb, 1e-3).clone()
    wrapped = ChannelEstimator("lin", p, cfo=comp)(sb, 1e-3).clone()
    eps = comp.estimate(sb).clone()
    flat = dataclasses.replace(sb, h_hat=comp.rotate(sb.h_hat.clone(), eps, _lib.CFO_REF_ZERO, -1))
    hand = comp.rotate(ChannelEstimator("lin", p)(flat, 1e-3), eps, _lib.CFO_REF_ZERO, +1)
    per_call = ChannelEstimator("lin", p)(sb, 1e-3, cfo=comp)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(wrapped.cpu().numpy(), hand.cpu().numpy())
    np.testing.assert_array_equal(per_call.cpu().numpy(), hand.cpu().numpy())
    np.testing.assert_array_equal(sb.h_hat.cpu().numpy(), g["h_hat"])          # the batch is left alone
    h, act = g["h"], g["active"]
    n_plain, n_wrapped = R.nmse(plain.cpu().numpy(), h, act), R.nmse(wrapped.cpu().numpy(), h, act)
    print("lin NMSE plain / wrapped:", n_plain, n_wrapped)
    assert n_wrapped < n_plain


@pytest.mark.parametrize("comp", [False, True])
def test_evaluate_cli_with_cfo(comp, capsys):
    from neural_rx_amd import evaluate
    names = ["lsnn_lmmse", "lslin_lmmse", "lmmse_lmmse", "perf_csi_lmmse"]
    argv = ["-config_name", "nrx_rt", "-num_tx_eval", "2", "-num_prbs", "4", "-ebno_db", "10", "-batch_size", "16",
            "-max_mc_iter", "2", "-num_cov_slots", "64", "-cfo_hz", "300", "-cfo_constant", "-baselines"] + names
    d = evaluate.main(argv + (["-cfo_comp"] if comp else []))
    c = d["cfo"]
    assert c["cfo_hz"] == 300.0 and c["constant"] is True and c["comp"] is comp and c["h_with_phase"] is True
    assert c["cfo_ppm"] is None and c["carrier_frequency_hz"] == 2.14e9
    # no accuracy is asked of the estimate here (the channel's own Doppler turns the pilots too):
    # |eps_hat| <= 1 / (2 * 1.07 * 9) = 0.0519 by construction and eps = 0.01
    assert len(c["eps_rms_error"]) == 1 and 0.0 <= c["eps_rms_error"][0] <= 0.0519 + 0.01
    assert d["mc_iters"] == [2] and list(d["baselines"]) == names
    for n in names:
        assert d["baselines"][n]["counts"][0][1] == d["counts"][0][1]      # paired: the same bits
    print("BER:", d["ber"][0], {n: d["baselines"][n]["ber"][0] for n in names}, "eps rms", c["eps_rms_error"])


def test_evaluate_cli_cfo_ppm():
    from neural_rx_amd import evaluate
    d = evaluate.main(["-config_name", "nrx_rt", "-num_prbs", "4", "-ebno_db", "10", "-batch_size", "8", "-max_mc_iter",
                       "1", "-cfo_ppm", "0.1"])
    assert abs(d["cfo"]["cfo_hz"] - 214.0) < 1e-9 and d["cfo"]["constant"] is False and d["cfo"]["comp"] is False
    plain = evaluate.main(["-config_name", "nrx_rt", "-num_prbs", "4", "-ebno_db", "10", "-batch_size", "8",
                           "-max_mc_iter", "1"])
    assert "cfo" not in plain
