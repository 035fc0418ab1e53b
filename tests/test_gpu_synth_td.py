"""The slot generator's time-domain transmit stage (``nrx_generate_slots_td``) on the GPU against the numpy
statement tests/ofdm_ref.py (needs an MI355X).  B = 3, U = 2, F = 48, A = 2, N = 64, cyclic prefix (6, 4, ..., 4).

Tolerances: x_out, y, h and h_hat within the generator's bound of tests/test_gpu_synth.py, 1e-6 relative to
max |.| plus 1e-7 absolute: both sides compute in f64 (the FFTs' own error is O(2^-52 log2 N)), y / h / h_hat
round once to f32.  bits, mcs, active, mcs_mask: the bits.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from oracle import synth_ref as S
from tests import ofdm_ref as O

pytestmark = pytest.mark.gpu

B, U, F, A, N = 3, 2, 48, 2, 64
CP = tuple([6] + [4] * 13)
NO, OFF = 0.02, 7
KEYS = ("y", "h_hat", "h", "active", "mcs_mask", "mcs", "bits")


def _params(td=None, **kw):
    from neural_rx_amd.generator import GenParams
    base = dict(num_tx=U, num_subcarriers=F, num_rx_ant=A, cdm_group=(0, 1), mcs_bits=(2, 4), mcs_of_user=(-1, 1),
                seed=53, td=td)
    base.update(kw)
    return GenParams(**base)


def _td(**kw):
    from neural_rx_amd.generator import TimeDomain
    return TimeDomain(fft_size=N, cp=list(CP), **kw)


def _spec(p, batch, no, off):
    return S.GenSpec(batch=batch, num_tx=p.num_tx, num_subcarriers=p.num_subcarriers, num_rx_ant=p.num_rx_ant,
                     dmrs_symbols=p.dmrs_symbols, cdm_group=p.cdm_group, mcs_bits=p.mcs_bits,
                     mcs_of_user=p.mcs_of_user, num_active=p.num_active, num_taps=p.num_taps,
                     num_sinusoids=p.num_sinusoids, max_delay_s=p.max_delay_s, max_doppler_hz=p.max_doppler_hz,
                     subcarrier_spacing=p.subcarrier_spacing, no=no, seed=p.seed, slot_offset=off)


@functools.lru_cache(maxsize=None)
def _base(batch=B, off=OFF):
    return S.generate(_spec(_params(), batch, NO, off))


def _host(sb):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in vars(sb).items() if v is not None}


def _gpu(p, batch=B, off=OFF):
    from neural_rx_amd.generator import SlotGenerator
    return _host(SlotGenerator(p, want_h=True, want_x=True)(batch, NO, slot_offset=off))


def _close(a, b, name):
    scale = float(np.abs(b).max())
    err = float(np.abs(a.astype(np.complex128 if np.iscomplexobj(b) else np.float64) - b).max())
    print(name, "max error", err, "scale", scale)
    assert err <= 1e-6 * scale + 1e-7, (name, err, scale)


def _raw(entry, td=None):
    """nrx_generate_slots_cir, or nrx_generate_slots_td with td = NULL / a td, on the same arguments in a
    workspace of exactly the size asked for; (outputs, workspace bytes)"""
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
    tdp = ctypes.byref(td) if td is not None else None
    if entry == "cir":
        _lib.check(lib.nrx_gen_workspace_size_cir(ctypes.byref(d), None, None, None, ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        _lib.check(lib.nrx_generate_slots_cir(ctypes.byref(d), None, None, None, None, ctypes.byref(o), ws.data_ptr(),
                                              ws.numel(), st))
    else:
        _lib.check(lib.nrx_gen_workspace_size_td(ctypes.byref(d), None, None, None, tdp, ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        _lib.check(lib.nrx_generate_slots_td(ctypes.byref(d), None, None, None, None, tdp, ctypes.byref(o), ws.data_ptr(),
                                             ws.numel(), st))
    return _host(sb), n.value


def test_without_a_td_it_is_the_cir_entry_point():
    old, size = _raw("cir")
    new, size_new = _raw("td")
    assert size_new == size and set(new) == set(old) and len(old) == 11
    for k in old:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    assert np.abs(old["y"]).max() > 0.1


def test_a_neutral_td_changes_nothing_but_rounding():
    plain = _gpu(_params())
    g = _gpu(_params(_td()))
    for k in ("bits", "active", "mcs", "mcs_mask", "h"):
        np.testing.assert_array_equal(g[k], plain[k], err_msg=k)
    _close(g["y"], plain["y"].astype(np.float64), "y")
    _close(g["h_hat"], plain["h_hat"].astype(np.float64), "h_hat")
    _close(g["x_td"], _base().x, "x_out")
    # in a workspace of exactly the size asked for, with the Aerial outputs
    raw, size = _raw("td", _td().struct(U))
    assert size > _raw("cir")[1]
    for k in ("y", "h_hat", "h", "bits"):
        np.testing.assert_array_equal(raw[k], g[k], err_msg=k)
    np.testing.assert_array_equal(raw["y_real"], g["y"][..., :A])
    np.testing.assert_array_equal(raw["y_imag"], g["y"][..., A:])


# (delays, pa_ibo_db): inside the prefix, beyond it, the amplifier, both
STAGES = [((0, 3), None), ((0, 7), None), ((0, 0), 3.0), ((2, 7), 3.0)]


@pytest.mark.parametrize("delay,ibo", STAGES)
@pytest.mark.parametrize("h_with_delay", [False, True])
def test_stage_against_the_statement(delay, ibo, h_with_delay):
    td = _td(delay=delay, pa_ibo_db=ibo, h_with_delay=h_with_delay)
    g = _gpu(_params(td))
    base = _base()
    ref = O.generate(_spec(_params(), B, NO, OFF), N, CP, delay, pa_ibo_db=ibo, h_with_delay=h_with_delay, base=base)
    for k in ("active", "mcs", "bits"):
        np.testing.assert_array_equal(g[k], getattr(base, k), err_msg=k)
    _close(g["x_td"], ref.x_out, "x_out")
    _close(g["y"], ref.y.astype(np.float64), "y")
    _close(g["h_hat"], ref.h_hat.astype(np.float64), "h_hat")
    _close(g["h"], ref.h.astype(np.float64), "h")
    assert np.abs(ref.x_out - base.x).max() > 0.05          # the stage did something
    if h_with_delay:                                        # ... and h against the formula itself
        hc = lambda z: z[..., :A].astype(np.float64) + 1j * z[..., A:].astype(np.float64)  # noqa: E731
        kf = np.arange(F) + (N // 2 - F // 2) - N // 2
        for u in range(U):
            ramp = np.exp(-2j * np.pi * delay[u] * kf / N)
            _close(hc(g["h"][:, u]), hc(base.h[:, u]) * ramp[None, :, None, None], f"h[{u}]")
    else:
        np.testing.assert_array_equal(g["h"], base.h)
    if ibo is None and max(delay) <= min(CP):               # a delay inside the prefix is the ramp alone
        for u in range(U):
            _close(g["x_td"][:, u], base.x[:, u] * O.delay_ramp(F, N, delay[u])[None, :, None], f"ramp[{u}]")


def test_first_bin_moves_the_ramp():
    td = _td(delay=(0, 3), h_with_delay=True, first_bin=3)
    g = _gpu(_params(td))
    ref = O.generate(_spec(_params(), B, NO, OFF), N, CP, (0, 3), first_bin=3, h_with_delay=True, base=_base())
    _close(g["x_td"], ref.x_out, "x_out")
    _close(g["h"], ref.h.astype(np.float64), "h")
    _close(g["y"], ref.y.astype(np.float64), "y")


def test_repeat_calls_and_batch_splits_give_the_same_bits():
    p = _params(_td(delay=(1, 7), pa_ibo_db=3.0, h_with_delay=True), num_active=1)
    full, again = _gpu(p, 3, off=11), _gpu(p, 3, off=11)
    first, second = _gpu(p, 2, off=11), _gpu(p, 1, off=13)
    for k in KEYS + ("x_td",):
        np.testing.assert_array_equal(again[k], full[k], err_msg=k)
        np.testing.assert_array_equal(first[k], full[k][:2], err_msg=k)
        np.testing.assert_array_equal(second[k], full[k][2:], err_msg=k)
    inactive = full["active"] == 0
    assert inactive.any() and not full["x_td"][inactive].any()        # an inactive port stays silent


def test_td_with_a_cfo_is_refused():
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.generator import SlotGenerator
    gen = SlotGenerator(_params(_td(delay=(0, 3))))
    cfo = _lib.nrx_gen_cfo()
    cfo.cfo_hz[0] = 200.0
    gen._cfo = cfo
    with pytest.raises(_lib.NRXError) as e:
        gen(B, NO)
    assert e.value.code == _lib.NRX_ERR_INVALID_ARG and "one transmit-side stage" in str(e.value)
    with pytest.raises(ValueError):
        dataclasses.replace(_params(_td()), cfo_hz=200.0)
    torch.cuda.synchronize()
