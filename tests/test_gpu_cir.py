"""The channel-impulse-response replay on the GPU (``nrx_generate_slots_cir``, ``nrx_generate_taps``) against the
numpy statement tests/cir_ref.py (needs an MI355X).

Tolerances: y, h, h_hat and the Aerial lists within the generator's bound of tests/test_gpu_synth.py, 1e-6 relative
to max |.| plus 1e-7 absolute: both sides compute in f64 and round once to f32.  bits, mcs, active: the bits.
The round trip through ``nrx_generate_taps`` has a bound of its own, computed from the exported arrays
(test_round_trip_through_the_exported_taps).

Shapes.  The replay kernel stages 32 paths per chunk, owns 64 subcarriers (16 per wave) and 64 of the 14 A columns
per workgroup: L = 1, 5, 31, 32, 33, 130; F = 12, 24, 50 (one tile, ragged) and 70, 132 (two and three tiles);
A = 1, 3, 4 (one column group, ragged) and 5, 16 (two and four groups, the last one narrower).
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from oracle import synth_ref as S
from tests import cfo_ref as C
from tests import cir_ref as R
from tests import dmrs_ref as D

pytestmark = pytest.mark.gpu

FIELDS = ("y", "h_hat", "h", "active", "mcs_mask", "mcs", "bits")
SEL = {"index": R.SELECT_INDEX, "random": R.SELECT_RANDOM, "trajectory": R.SELECT_TRAJECTORY}


@functools.lru_cache(maxsize=None)
def _data(E, A, L, Ta, zero=None):
    """(a complex64 [E, A, L, Ta], tau float32 [E, L]): delay-dependent power, delays up to 1 us; ``zero``: an
    example without any energy"""
    rng = np.random.default_rng(1000 * E + 100 * A + L + Ta)
    tau = np.sort(rng.uniform(0.0, 1e-6, (E, L)), axis=-1).astype(np.float32)
    a = (rng.standard_normal((E, A, L, Ta)) + 1j * rng.standard_normal((E, A, L, Ta)))
    a = (a * np.exp(-tau.astype(np.float64) / 6e-7)[:, None, :, None]).astype(np.complex64)
    if zero is not None:
        a[zero] = 0
    return a, tau


def _params(U, F, A, cir, **kw):
    from neural_rx_amd.generator import GenParams
    base = dict(num_tx=U, num_subcarriers=F, num_rx_ant=A, cdm_group=tuple(u % 2 for u in range(U)), mcs_bits=(2, 4),
                mcs_of_user=tuple(-1 if u % 2 == 0 else 1 for u in range(U)), seed=47, cir=cir)
    base.update(kw)
    return GenParams(**base)


def _channel(a, tau, select="random", normalize=True, f_offset="centered"):
    from neural_rx_amd.cir import CIRChannel, CIRDataset
    return CIRChannel(CIRDataset(a, tau), select=select, normalize=normalize, f_offset=f_offset)


def _spec(p, batch, no, off=0):
    return S.GenSpec(batch=batch, num_tx=p.num_tx, num_subcarriers=p.num_subcarriers, num_rx_ant=p.num_rx_ant,
                     dmrs_symbols=p.dmrs_symbols, cdm_group=p.cdm_group, mcs_bits=p.mcs_bits,
                     mcs_of_user=p.mcs_of_user, num_active=p.num_active, num_taps=p.num_taps,
                     num_sinusoids=p.num_sinusoids, max_delay_s=p.max_delay_s, max_doppler_hz=p.max_doppler_hz,
                     subcarrier_spacing=p.subcarrier_spacing, no=no, seed=p.seed, slot_offset=off)


def _ref(p, batch, no, off=0, index=None):
    ch = p.cir
    return R.generate(_spec(p, batch, no, off), ch.dataset.a, ch.dataset.tau, SEL[ch.select], index,
                      ch.normalize, ch.offset(p.num_subcarriers))


def _host(sb):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in vars(sb).items() if v is not None}


def _gpu(p, batch, no, off=0, aerial=False, index=None):
    import torch
    from neural_rx_amd.generator import SlotGenerator
    idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).cuda() if index is not None else None
    return _host(SlotGenerator(p, want_h=True, aerial=aerial)(batch, no, slot_offset=off, cir_index=idx))


def _close(a, b, name):
    scale = float(np.abs(b).max())
    err = float(np.abs(a.astype(np.float64) - b).max())
    print(name, "max error", err, "scale", scale)
    assert err <= 1e-6 * scale + 1e-7, (name, err, scale)


def _parity(p, B, no=0.02, off=7, index=None):
    aerial = p.num_subcarriers % 12 == 0
    g = _gpu(p, B, no, off, aerial=aerial, index=index)
    o, H, e = _ref(p, B, no, off, index)
    for k in ("active", "mcs", "bits"):
        np.testing.assert_array_equal(g[k], getattr(o, k))
    _close(g["y"], o.y, "y")
    _close(g["h"], o.h, "h")
    _close(g["h_hat"], o.h_hat, "h_hat")
    if aerial:
        A = p.num_rx_ant
        _close(g["y_real"], o.y[..., :A], "y_real")
        _close(g["y_imag"], o.y[..., A:], "y_imag")
        hr, hi = C.aerial_pilots(o.h_hat, p.dmrs_symbols, p.cdm_group)
        _close(g["h_ls_real"], hr, "h_ls_real")
        _close(g["h_ls_imag"], hi, "h_ls_imag")
    return g, o, H, e


# (F, A, U, L, Ta, B, select, E, normalize, f_offset)
PARITY = [
    (12, 1, 1, 1, 1, 2, "random", 1, False, "zero"),
    (24, 3, 2, 5, 14, 3, "trajectory", 7, True, "centered"),
    (50, 4, 3, 31, 14, 2, "random", 7, True, "centered"),
    (24, 4, 2, 32, 1, 3, "trajectory", 7, False, "zero"),
    (50, 3, 1, 33, 14, 2, "random", 7, True, "zero"),
    (24, 4, 3, 130, 1, 2, "random", 7, True, "centered"),
    (12, 1, 2, 130, 14, 2, "trajectory", 7, False, "centered"),
    (132, 5, 2, 33, 14, 1, "random", 7, True, "centered"),
    (70, 16, 1, 5, 1, 1, "random", 1, True, "zero"),
    (50, 4, 2, 32, 14, 2, "random", 7, False, -3.5),
]


@pytest.mark.parametrize("F,A,U,L,Ta,B,select,E,normalize,f_offset", PARITY)
def test_replay_matches_reference(F, A, U, L, Ta, B, select, E, normalize, f_offset):
    a, tau = _data(E, A, L, Ta)
    p = _params(U, F, A, _channel(a, tau, select, normalize, f_offset))
    g, o, H, e = _parity(p, B)
    assert np.abs(o.h).max() > 1e-2
    if normalize:
        c = np.mean(np.abs(H) ** 2, axis=(2, 3, 4))
        assert np.abs(c - 1.0).max() < 1e-12
    if select == "trajectory":
        np.testing.assert_array_equal(e % U, np.broadcast_to(np.arange(U), e.shape))


@pytest.mark.parametrize("normalize", [False, True])
def test_index_selection_and_entries_outside_the_dataset(normalize):
    """-1 and E give that user an exactly zero h and no contribution to y; example 2 has no energy at all"""
    E, A, L, U, F, B = 7, 3, 33, 2, 24, 3
    a, tau = _data(E, A, L, 14, zero=2)
    index = np.array([[0, -1], [E, 3], [6, 2]], np.int32)
    p = _params(U, F, A, _channel(a, tau, "index", normalize, "centered"))
    g, o, H, e = _parity(p, B, index=index)
    np.testing.assert_array_equal(e, [[0, -1], [-1, 3], [6, 2]])
    for b, u in ((0, 1), (1, 0), (2, 1)):
        assert (g["h"][b, u] == 0).all() and (o.h[b, u] == 0).all(), (b, u)
    # y of slot 0 is user 0 alone: the reference without user 1 is the same y
    solo = np.einsum("aft,ft->aft", H[0, 0], o.x[0, 0]) + R.noise(_spec(p, B, 0.02, 7))[0]
    _close(g["y"][0], R.to_ch(solo), "y of the slot with a zero-channel user")
    assert np.abs(g["h"][0, 0]).max() > 1e-2 and np.abs(g["h"][2, 0]).max() > 1e-2


def test_composition_with_a_carrier_frequency_offset():
    a, tau = _data(7, 2, 33, 14)
    p = _params(2, 36, 2, _channel(a, tau, "random", True, "centered"), cfo_hz=(900.0, 2400.0), cfo_constant=True,
                fft_size=64, h_with_phase=True)
    B, no, off = 3, 0.02, 7
    g = _gpu(p, B, no, off)
    base, _, _ = _ref(p, B, no, off)
    o = C.generate(_spec(p, B, no, off), p.cfo_per_port(), True, 64, True, base=base)
    np.testing.assert_array_equal(g["cfo_eps"], o.eps)
    np.testing.assert_array_equal(g["bits"], base.bits)
    _close(g["y"], o.y, "y")
    _close(g["h_hat"], o.h_hat, "h_hat")
    _close(g["h"], o.h, "h")
    assert np.abs(o.y - base.y).max() > 1e-3 and np.abs(o.h - base.h).max() > 1e-3


def test_composition_with_cover_coded_ports():
    from neural_rx_amd.ls import DMRSPorts
    U, F, A, B, no, off = 4, 24, 3, 2, 0.02, 7
    ports = DMRSPorts.default(U)
    assert ports.despread_f and not ports.despread_t
    tup = (list(ports.cdm_group), list(ports.focc), list(ports.tocc))
    a, tau = _data(7, A, 33, 14)
    p = _params(U, F, A, _channel(a, tau, "random", True, "centered"), dmrs=ports, num_active=3)
    g = _gpu(p, B, no, off, aerial=True)
    s = _spec(p, B, no, off)
    base, H, _ = _ref(p, B, no, off)
    r = D.base_sequence(p.seed, F, len(p.dmrs_symbols))
    dm = np.zeros(14, bool)
    dm[list(p.dmrs_symbols)] = True
    x2 = np.where(dm[None, None, None, :], D.port_pilots(r, tup, F, p.dmrs_symbols)[None] * base.active[:, :, None, None],
                  base.x)
    y = R.to_ch(np.einsum("buaft,buft->baft", H, x2) + R.noise(s))
    h_ls, h_pair = D.ls_estimate(y, D.pilot_table(r), p.dmrs_symbols, tup, True, False, base.active)
    np.testing.assert_array_equal(g["active"], base.active)
    np.testing.assert_array_equal(g["bits"], base.bits)
    np.testing.assert_array_equal(g["pilots"], D.pilot_table(r))
    _close(g["y"], y, "y")
    _close(g["h"], base.h, "h")
    _close(g["h_hat"], D.h_hat(h_ls, tup, F, p.dmrs_symbols), "h_hat")
    hr, hi = D.aerial_list(h_pair, F)
    _close(g["h_ls_real"], hr, "h_ls_real")
    _close(g["h_ls_imag"], hi, "h_ls_imag")
    assert np.abs(y - base.y).max() > 1e-2


def _raw(p, batch, no, entry, off=3):
    """nrx_generate_slots_cir with cir = NULL, or nrx_generate_slots_dmrs, on the same arguments (a CFO and cover-coded
    ports) in a workspace of exactly the size asked for; (outputs, workspace bytes)"""
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.generator import SlotGenerator
    lib = _lib.load()
    gen = SlotGenerator(p, want_h=True, aerial=True)
    sb = gen._alloc(batch)
    for v in vars(sb).values():
        if v is not None:
            v.zero_()
    d = p.desc(batch, no, off)
    o = _lib.nrx_gen_out()
    o.y, o.h_hat, o.h, o.active = (t.data_ptr() for t in (sb.y, sb.h_hat, sb.h, sb.active))
    o.mcs_mask, o.mcs, o.bits, o.bits_stride = sb.mcs_mask.data_ptr(), sb.mcs.data_ptr(), sb.bits.data_ptr(), p.bits_max
    o.y_real, o.y_imag, o.h_ls_real, o.h_ls_imag = (t.data_ptr() for t in (sb.y_real, sb.y_imag, sb.h_ls_real, sb.h_ls_imag))
    gen._cfo.eps_out, gen._dmrs.pilots_out = sb.cfo_eps.data_ptr(), sb.pilots.data_ptr()
    cfo, dmrs = ctypes.byref(gen._cfo), ctypes.byref(gen._dmrs)
    n = ctypes.c_size_t()
    st = torch.cuda.current_stream().cuda_stream
    if entry == "dmrs":
        _lib.check(lib.nrx_gen_workspace_size_dmrs(ctypes.byref(d), cfo, dmrs, ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        _lib.check(lib.nrx_generate_slots_dmrs(ctypes.byref(d), None, cfo, dmrs, ctypes.byref(o), ws.data_ptr(), ws.numel(), st))
    else:
        _lib.check(lib.nrx_gen_workspace_size_cir(ctypes.byref(d), cfo, dmrs, None, ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        _lib.check(lib.nrx_generate_slots_cir(ctypes.byref(d), None, cfo, dmrs, None, ctypes.byref(o), ws.data_ptr(),
                                              ws.numel(), st))
    return _host(sb), n.value


def test_without_a_cir_it_is_the_dmrs_entry_point():
    from neural_rx_amd.ls import DMRSPorts
    p = _params(4, 24, 3, None, dmrs=DMRSPorts.default(4), cfo_hz=(900.0, 0.0, 300.0, 50.0))
    old, size = _raw(p, 3, 0.05, "dmrs")
    new, size_new = _raw(p, 3, 0.05, "cir")
    assert size_new == size
    assert set(new) == set(old) and len(old) == 13
    for k in old:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    assert np.abs(old["y"]).max() > 0.1


@pytest.mark.parametrize("select", ["random", "trajectory"])
def test_repeat_calls_and_batch_splits_give_the_same_bits(select):
    a, tau = _data(7, 4, 33, 14)
    p = _params(2, 50, 4, _channel(a, tau, select, True, "centered"), num_active=1)
    keys = ("y", "h_hat", "h", "active", "mcs", "bits")
    full, again = _gpu(p, 4, 0.05, off=11), _gpu(p, 4, 0.05, off=11)
    first, second = _gpu(p, 2, 0.05, off=11), _gpu(p, 2, 0.05, off=13)
    for k in keys:
        np.testing.assert_array_equal(again[k], full[k], err_msg=k)
        np.testing.assert_array_equal(first[k], full[k][:2], err_msg=k)
        np.testing.assert_array_equal(second[k], full[k][2:], err_msg=k)
    # the slots are not all on one example
    assert len({full["h"][b, 0].tobytes() for b in range(4)}) > 1


def test_bits_mcs_and_active_are_those_of_the_built_in_channel():
    a, tau = _data(7, 4, 5, 1)
    p = _params(3, 24, 4, _channel(a, tau), num_active=2)
    g = _gpu(p, 3, 0.05, off=2)
    plain = _gpu(dataclasses.replace(p, cir=None), 3, 0.05, off=2)
    for k in ("bits", "mcs", "active", "mcs_mask"):
        np.testing.assert_array_equal(g[k], plain[k], err_msg=k)
    assert np.abs(g["y"] - plain["y"]).max() > 1e-2


def test_round_trip_through_the_exported_taps():
    """nrx_generate_taps, then a replay by index with f_offset 0 and no normalisation, against nrx_generate_slots.
    One f32 rounding of every tap and delay, |d h| <= 2^-24 sum_l |g_l| (1 + 2 pi f scs tau_l), one of each side's result,
    2^-24 |h| each -- so |h_replay - h| <= 2 2^-24 (sum_l |g_l(t)| (1 + 2 pi f scs tau_l) + |h|), the factor 2 on the
    first term left as slack; y: that bound through sum_u |x_u| plus 2 2^-24 |y| of its own."""
    import torch
    from neural_rx_amd.cir import CIRChannel
    from neural_rx_amd.generator import SlotGenerator
    B, U, F, A, L, no, off = 3, 2, 48, 4, 6, 0.02, 9
    p = _params(U, F, A, None, num_taps=L)
    gen = SlotGenerator(p, want_h=True)
    built_in = _host(gen(B, no, slot_offset=off))
    ds = gen.export_taps(B, slot_offset=off)
    torch.cuda.synchronize()
    a, tau = ds.a.cpu().numpy(), ds.tau.cpu().numpy()
    assert a.shape == (B * U, A, L, 14) and a.dtype == np.complex64 and tau.shape == (B * U, L) and tau.dtype == np.float32
    s = _spec(p, B, no, off)
    gt, t64 = R.oracle_taps(s)
    want_a, want_tau, index = R.as_dataset(gt, t64)
    _close(np.stack([a.real, a.imag], -1), np.stack([want_a.real, want_a.imag], -1).astype(np.float32), "exported taps")
    _close(tau, want_tau.astype(np.float32), "exported delays")
    q = dataclasses.replace(p, cir=CIRChannel(ds, select="index", normalize=False, f_offset="zero"))
    g = _gpu(q, B, no, off, index=index)
    for k in ("bits", "mcs", "active"):
        np.testing.assert_array_equal(g[k], built_in[k])
    u24 = 2.0 ** -24
    f = np.arange(F, dtype=np.float64)
    w = 1.0 + 2.0 * np.pi * f[None, :] * p.subcarrier_spacing * tau.astype(np.float64)[:, :, None]      # [E, L, F]
    first = np.einsum("ealt,elf->eaft", np.abs(a.astype(np.complex128)), w).reshape(B, U, A, F, 14)
    cplx = lambda z: z[..., :A].astype(np.float64) + 1j * z[..., A:].astype(np.float64)  # noqa: E731
    h0, h1 = cplx(built_in["h"]), cplx(g["h"])                               # [B, U, F, T, A]
    bound_h = 2.0 * u24 * (np.moveaxis(first, 2, -1) + np.abs(h0))
    excess = np.abs(h1 - h0) / bound_h
    print("round trip h: max |dh| / bound", excess.max())
    assert (np.abs(h1 - h0) <= bound_h).all()
    x = np.abs(S.generate(s).x)                                              # [B, U, F, T]
    y0, y1 = cplx(built_in["y"]), cplx(g["y"])                               # [B, F, T, A]
    bound_y = np.einsum("bufta,buft->bfta", bound_h, x) + 2.0 * u24 * np.abs(y0)
    print("round trip y: max |dy| / bound", (np.abs(y1 - y0) / bound_y).max())
    assert (np.abs(y1 - y0) <= bound_y).all()
    assert np.abs(h0).max() > 0.1
