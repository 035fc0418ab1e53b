"""The slot generator with the time-domain channel (``nrx_generate_slots_tc``) on the GPU against the numpy
statement tests/timechan_ref.py (needs an MI355X).  B = 3, U = 2, F = 48, A = 2, N = 64, cyclic prefix (6, 4, ..., 4),
L = 3 paths of NS = 4 sinusoids, fs = 64 * 30 kHz.

Tolerances: y, h, h_hat and r_out within the generator's bound of tests/test_gpu_synth.py, 1e-6 relative to
max |.| plus 1e-7 absolute: both sides compute in f64, y / h / h_hat round once to f32.  bits, mcs, active,
mcs_mask: the bits.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import synth_ref as S
from tests import dmrs_ref as D
from tests import synth_chan_ref as C
from tests import timechan_ref as R

pytestmark = pytest.mark.gpu

B, U, F, A, N = 3, 2, 48, 2, 64
CP = tuple([6] + [4] * 13)
FS = N * 30e3
NO, OFF = 0.02, 7
KEYS = ("y", "h_hat", "h", "active", "mcs_mask", "mcs", "bits")


def _params(tc=None, **kw):
    from neural_rx_amd.generator import GenParams
    base = dict(num_tx=U, num_subcarriers=F, num_rx_ant=A, cdm_group=(0, 1), mcs_bits=(2, 4), mcs_of_user=(-1, 1),
                num_taps=3, num_sinusoids=4, seed=53, tc=tc)
    base.update(kw)
    return GenParams(**base)


def _tc(**kw):
    from neural_rx_amd.generator import TimeChannelParams
    return TimeChannelParams(fft_size=N, cp=list(CP), **kw)


def _spec(p, batch=B, no=NO, off=OFF):
    return S.GenSpec(batch=batch, num_tx=p.num_tx, num_subcarriers=p.num_subcarriers, num_rx_ant=p.num_rx_ant,
                     dmrs_symbols=p.dmrs_symbols, cdm_group=p.cdm_group, mcs_bits=p.mcs_bits,
                     mcs_of_user=p.mcs_of_user, num_active=p.num_active, num_taps=p.num_taps,
                     num_sinusoids=p.num_sinusoids, max_delay_s=p.max_delay_s, max_doppler_hz=p.max_doppler_hz,
                     subcarrier_spacing=p.subcarrier_spacing, no=no, seed=p.seed, slot_offset=off)


def _host(sb):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in vars(sb).items() if v is not None}


def _gpu(p, batch=B, off=OFF, aerial=False):
    from neural_rx_amd.generator import SlotGenerator
    return _host(SlotGenerator(p, want_h=True, want_r=True, aerial=aerial)(batch, NO, slot_offset=off))


def _close(a, b, name):
    scale = float(np.abs(b).max())
    err = float(np.abs(a.astype(np.complex128 if np.iscomplexobj(b) else np.float64) - b).max())
    print(name, "max error", err, "scale", scale)
    assert err <= 1e-6 * scale + 1e-7, (name, err, scale)


def _against(g, ref, plain):
    for k in ("active", "mcs", "bits", "mcs_mask"):
        np.testing.assert_array_equal(g[k], plain[k], err_msg=k)
    np.testing.assert_array_equal(g["active"], ref.base.active)
    np.testing.assert_array_equal(g["bits"], ref.base.bits)
    _close(g["r_tc"], ref.r, "r_out")
    _close(g["y"], ref.y.astype(np.float64), "y")
    _close(g["h"], ref.h.astype(np.float64), "h")
    _close(g["h_hat"], ref.h_hat.astype(np.float64), "h_hat")


def _raw(entry, tc=None, x_out=None):
    """nrx_generate_slots_td, or nrx_generate_slots_tc with tc = NULL / a tc, on the same arguments in a workspace
    of exactly the size asked for; (outputs, workspace bytes).  ``x_out``: a device tensor for tc.x_out"""
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.generator import SlotGenerator
    lib = _lib.load()
    p = _params()
    sb = SlotGenerator(p, want_h=True, aerial=True)._alloc(B)
    for v in vars(sb).values():
        if v is not None:
            v.zero_()
    d = p.desc(B, NO, OFF)
    o = _lib.nrx_gen_out()
    o.y, o.h_hat, o.h, o.active = (t.data_ptr() for t in (sb.y, sb.h_hat, sb.h, sb.active))
    o.mcs_mask, o.mcs, o.bits, o.bits_stride = sb.mcs_mask.data_ptr(), sb.mcs.data_ptr(), sb.bits.data_ptr(), p.bits_max
    o.y_real, o.y_imag, o.h_ls_real, o.h_ls_imag = (t.data_ptr() for t in (sb.y_real, sb.y_imag, sb.h_ls_real, sb.h_ls_imag))
    n = ctypes.c_size_t()
    st = torch.cuda.current_stream().cuda_stream
    if x_out is not None:
        tc.x_out = x_out.data_ptr()
    tcp = ctypes.byref(tc) if tc is not None else None
    if entry == "td":
        _lib.check(lib.nrx_gen_workspace_size_td(ctypes.byref(d), None, None, None, None, ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        _lib.check(lib.nrx_generate_slots_td(ctypes.byref(d), None, None, None, None, None, ctypes.byref(o),
                                             ws.data_ptr(), ws.numel(), st))
    else:
        _lib.check(lib.nrx_gen_workspace_size_tc(ctypes.byref(d), None, None, None, None, None, tcp, ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        _lib.check(lib.nrx_generate_slots_tc(ctypes.byref(d), None, None, None, None, None, tcp, ctypes.byref(o),
                                             ws.data_ptr(), ws.numel(), st))
    return _host(sb), n.value


def test_without_a_tc_it_is_the_td_entry_point():
    old, size = _raw("td")
    new, size_new = _raw("tc")
    assert size_new == size and set(new) == set(old) and len(old) == 11
    for k in old:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    assert np.abs(old["y"]).max() > 0.1


@functools.lru_cache(maxsize=None)
def _plain(doppler, delay):
    return _gpu(_params(max_doppler_hz=doppler, max_delay_s=delay))


# (max_doppler_hz, max_delay_s, l_min, l_max, timing advance): static and inside the prefix; a Doppler of 20 kHz;
# a delay beyond the prefix (the default l_max = 12 + 6)
CHANNELS = [(0.0, 300e-9, -2, 2, 2), (20e3, 300e-9, -6, None, 0), (400.0, 12 / FS, -6, None, 0)]


@pytest.mark.parametrize("doppler,delay,l_min,l_max,ta", CHANNELS)
def test_channel_against_the_statement(doppler, delay, l_min, l_max, ta):
    p = _params(_tc(l_min=l_min, l_max=l_max, timing_advance=ta), max_doppler_hz=doppler, max_delay_s=delay)
    g = _gpu(p)
    ref = R.generate(_spec(p), N, CP, l_min, -1 if l_max is None else l_max, ta)
    _against(g, ref, _plain(doppler, delay))
    hx = np.einsum("buaft,buft->baft", ref.h_c, ref.base.x)
    res = float(np.abs(ref.y_free - hx).max() / np.abs(hx).max())
    print("interference over the diagonal channel:", res)
    if doppler == 0.0:
        # the realisation of the plain generator up to the sinc truncation, and no interference
        assert res < 1e-12
        assert np.abs(g["h"] - _plain(doppler, delay)["h"]).max() < 0.2 * np.abs(g["h"]).max()
    else:
        assert res > 1e-3


# (A, F): the block shapes of k_tc_h, FB = min(4, 256 / (14 A)) subcarriers per workgroup.  The shapes above run
# FB = 4 with F % FB == 0 only.  A = 5: FB = 3, 17 workgroups, the last with two subcarriers (the ff < F and f >= F
# guards); A = 16: FB = 1; A = 8: FB = 2.  A = 5 and 8 also take the generator through k_timechan<8, 2>, A = 16
# through <16, 1>.  An MI355X run: y, h and h_hat equal the statement's f32 values bit for bit at all three shapes;
# r_out within 2.8e-14, 3.8e-14 and 3.5e-14 of it (scale 5.4 to 6.4).
H_BLOCKS = [(5, 50), (16, 48), (8, 46)]


@pytest.mark.parametrize("A_,F_", H_BLOCKS)
def test_channel_against_the_statement_at_other_block_shapes(A_, F_):
    doppler, delay = 20e3, 300e-9
    kw = dict(num_rx_ant=A_, num_subcarriers=F_, max_doppler_hz=doppler, max_delay_s=delay)
    p = _params(_tc(l_min=-6, l_max=None, timing_advance=0), **kw)
    g = _gpu(p)
    assert g["h"].shape == (B, U, F_, 14, 2 * A_)
    ref = R.generate(_spec(p), N, CP, -6, -1, 0)
    _against(g, ref, _gpu(_params(**kw)))


def test_exact_workspace_and_aerial_outputs():
    p = _params(_tc())
    g = _gpu(p)
    import torch
    xs = torch.zeros((B, U, p.tc.num_samples()), dtype=torch.complex128, device="cuda")
    raw, size = _raw("tc", p.tc.struct(), x_out=xs)
    assert size > _raw("td")[1]
    _close(xs.cpu().numpy(), R.generate(_spec(p), N, CP).xs, "x_out")        # the transmitted samples
    for k in ("y", "h_hat", "h", "bits"):
        np.testing.assert_array_equal(raw[k], g[k], err_msg=k)
    np.testing.assert_array_equal(raw["y_real"], g["y"][..., :A])
    np.testing.assert_array_equal(raw["y_imag"], g["y"][..., A:])
    assert np.abs(raw["h_ls_real"]).max() > 0.01


def test_per_port_profiles_and_an_antenna_mix():
    prof = [(300e-9, 400.0), (2e-6, 5e3)]
    p = _params(_tc(timing_advance=1, first_bin=3), user_profiles=prof, rx_corr=C.random_psd(A, 3))
    g = _gpu(p)
    ref = R.generate(_spec(p), N, CP, -6, -1, 1, first_bin=3, user_profiles=prof, rx_mix=p.rx_mix())
    _against(g, ref, _gpu(_params(user_profiles=prof, rx_corr=C.random_psd(A, 3))))
    unmixed = R.generate(_spec(p), N, CP, -6, -1, 1, first_bin=3, user_profiles=prof, base=ref.base)
    assert np.abs(unmixed.r - ref.r).max() > 0.05            # the mix did something


def test_with_cover_coded_dmrs_ports():
    from neural_rx_amd.ls import DMRSPorts
    ports = DMRSPorts.from_ports([0, 1])                       # one CDM group, told apart by the frequency cover
    tup = (list(ports.cdm_group), list(ports.focc), list(ports.tocc))
    p = _params(_tc(l_min=-2, l_max=2, timing_advance=2), dmrs=ports, max_doppler_hz=0.0)
    g = _gpu(p)
    s = _spec(p)
    base = S.generate(s)
    r = D.base_sequence(p.seed, F, len(p.dmrs_symbols))
    dm = np.zeros(14, bool)
    dm[list(p.dmrs_symbols)] = True
    x2 = np.where(dm[None, None, None, :], D.port_pilots(r, tup, F, p.dmrs_symbols)[None] * base.active[:, :, None, None],
                  base.x)
    ref = R.generate(s, N, CP, -2, 2, 2, base=base, x=x2)
    h_ls, _ = D.ls_estimate(ref.y, D.pilot_table(r), p.dmrs_symbols, tup, True, False, base.active)
    np.testing.assert_array_equal(g["bits"], base.bits)
    np.testing.assert_array_equal(g["pilots"], D.pilot_table(r))
    _close(g["r_tc"], ref.r, "r_out")
    _close(g["y"], ref.y.astype(np.float64), "y")
    _close(g["h"], ref.h.astype(np.float64), "h")
    _close(g["h_hat"], D.h_hat(h_ls, tup, F, p.dmrs_symbols), "h_hat")
    assert np.abs(x2 - base.x).max() > 0.5


def test_refusals():
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.generator import GenParams, SlotGenerator, TimeChannelParams, TimeDomain
    gen = SlotGenerator(_params(_tc()))
    cfo = _lib.nrx_gen_cfo()
    cfo.cfo_hz[0] = 200.0
    gen._cfo = cfo
    with pytest.raises(_lib.NRXError) as e:
        gen(B, NO)
    assert e.value.code == _lib.NRX_ERR_INVALID_ARG and "one sample-domain stage" in str(e.value)
    gen = SlotGenerator(_params(_tc()))
    gen._td = TimeDomain(fft_size=N, cp=list(CP)).struct(U)
    with pytest.raises(_lib.NRXError) as e:
        gen(B, NO)
    assert e.value.code == _lib.NRX_ERR_INVALID_ARG and "one sample-domain stage" in str(e.value)
    for kw in (dict(cfo_hz=200.0), dict(td=TimeDomain(fft_size=N))):
        with pytest.raises(ValueError, match="one sample-domain stage"):
            GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A, tc=TimeChannelParams(N), **kw)
    with pytest.raises(_lib.NRXError) as e:                    # a span beyond 256 taps
        SlotGenerator(_params(_tc(l_min=-200, l_max=200)))(B, NO)
    assert e.value.code == -2 and "span" in str(e.value)
    torch.cuda.synchronize()


def test_repeat_calls_and_batch_splits_give_the_same_bits():
    p = _params(_tc(timing_advance=1), num_active=1, max_doppler_hz=5e3)
    full, again = _gpu(p, 3, off=11), _gpu(p, 3, off=11)
    first, second = _gpu(p, 2, off=11), _gpu(p, 1, off=13)
    for k in KEYS + ("r_tc",):
        np.testing.assert_array_equal(again[k], full[k], err_msg=k)
        np.testing.assert_array_equal(first[k], full[k][:2], err_msg=k)
        np.testing.assert_array_equal(second[k], full[k][2:], err_msg=k)


def test_an_inactive_port_contributes_nothing():
    """with one active port per slot, r_out is that port's signal alone: the statement with the other port's
    draws but a silent x"""
    p = _params(_tc(), num_active=1, max_doppler_hz=5e3)
    g = _gpu(p, off=11)
    s = _spec(p, off=11)
    ref = R.generate(s, N, CP, -6, -1, 0)
    assert (g["active"] == 0).any() and (g["active"].sum(1) == 1).all()
    _close(g["r_tc"], ref.r, "r_out")
    tau, g0, fd = R.channel_draws(s, N)
    on = g["active"].astype(bool)
    alone = R.time_channel(ref.xs * on[:, :, None], tau * on[:, :, None], g0 * on[:, :, None, None, None], fd, FS,
                           CP[0], -6, 7)
    _close(g["r_tc"], alone, "r_out of the active port alone")
    h = g["h_hat"][~on]
    assert not h.any()


def test_evaluate_zero_doppler_is_paired_with_the_plain_run(capsys):
    """-tc_fft_size 64 -max_doppler_hz 0 next to the plain run: the same bits and noise on the same realisation
    up to the sinc truncation, so the perfect-CSI LMMSE BERs differ by no more than the two runs' binomial 3 sigma"""
    from neural_rx_amd import evaluate
    argv = ["-config_name", "nrx_rt", "-num_prbs", "2", "-ebno_db", "2", "-batch_size", "16", "-max_mc_iter", "2",
            "-baselines", "perf_csi_lmmse", "-max_doppler_hz", "0"]
    plain = evaluate.main(argv)
    tc = evaluate.main(argv + ["-tc_fft_size", "64"])
    assert set(tc) == set(plain) | {"tc"} and tc["tc"]["fft_size"] == 64 and tc["tc"]["max_doppler_hz"] == 0.0
    ber, var = [], 0.0
    for d in (plain, tc):
        err, bits = d["baselines"]["perf_csi_lmmse"]["counts"][0][:2]
        ber.append(err / bits)
        var += ber[-1] * (1.0 - ber[-1]) / bits
    with capsys.disabled():
        print("perfect-CSI LMMSE BER plain", ber[0], "time-domain channel", ber[1], "3 sigma", 3.0 * var ** 0.5)
    assert plain["baselines"]["perf_csi_lmmse"]["counts"][0][1] == tc["baselines"]["perf_csi_lmmse"]["counts"][0][1]
    assert 0.0 < ber[0] < 0.5 and abs(ber[1] - ber[0]) <= 3.0 * var ** 0.5
    capsys.readouterr()
