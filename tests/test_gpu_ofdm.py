"""nrx_ofdm_modulate / nrx_ofdm_demodulate on the GPU against the numpy statement tests/ofdm_ref.py (needs an
MI355X).  B = 2, S = 3 (odd, so the 2S axis of the CGNN layout is no multiple of 4).

Tolerances, err = max |out - ref| / max |ref| with ref the complex128 statement on the same inputs:
  f32   8 max(floor, 2^-23), floor = the same metric for the statement run in complex64 (numpy's FFT keeps single
        precision): the factor 8 is the margin this project uses over a numpy floor
  f64   8 2^-52 log2 N: both sides carry the FFT's O(eps log N) error
An error above a gate is a finding about the twiddles or the order of accumulation, not a reason to widen it.

Sizes.  N = 64, 128, 256, 512 run 16, 8, 4, 2 transforms per workgroup, 1024 one with one butterfly per thread,
2048 and 4096 one with 2 and 4; log2 N even (64, 256, 1024, 4096) is radix 4 alone, odd ends in a radix-2 pass.
F = N (no guard bins), 48, 25 (odd).  The cyclic prefix is (6, 4, ..., 4) N / 64, or 0.  Outputs are the NaN-
poisoned bodies of guarded buffers (tests/memguard.py): every element written, nothing beyond.
"""
import functools

import numpy as np
import pytest

from tests import memguard
from tests import ofdm_ref as O

pytestmark = pytest.mark.gpu

B, S = 2, 3
CDT = {"f32": np.complex64, "f64": np.complex128}


def _cp(N, kind, T=14):
    return [0] * T if kind == "zero" else ([6 * N // 64] + [4 * N // 64] * 13)[:T]


def _gate(N, precision, floor):
    return 8 * max(floor, 2.0 ** -23) if precision == "f32" else 8 * 2.0 ** -52 * np.log2(N)


def _err(a, ref):
    return float(np.abs(a.astype(np.complex128) - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def _grid(N, F, T, precision):
    rng = np.random.default_rng(N * 131 + F * 7 + T)
    g = (rng.standard_normal((B, S, F, T)) + 1j * rng.standard_normal((B, S, F, T))) / np.sqrt(2.0)
    g = g.astype(CDT[precision])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _samples(N, L, precision):
    rng = np.random.default_rng(N * 17 + L)
    s = ((rng.standard_normal((B, S, L)) + 1j * rng.standard_normal((B, S, L))) / np.sqrt(2.0)).astype(CDT[precision])
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _mod_ref(N, F, first_bin, cpk, T, precision, pad, asat=0.0):
    """(complex128 statement, floor of the complex64 one) on the inputs of that precision"""
    g = _grid(N, F, T, precision)
    cp = _cp(N, cpk, T)
    L = sum(cp) + T * N + pad
    ref = O.modulate(g, N, cp, first_bin, L=L, asat=asat)
    floor = _err(O.modulate(g, N, cp, first_bin, L=L, asat=asat, dtype=np.complex64), ref) if precision == "f32" else 0.0
    ref.setflags(write=False)
    return ref, floor


def _offsets(N, kind):
    return {"zero": (0, 0, 0), "mixed": (-(N // 2) - 3, 5, 0), "far": (-20 * N, 1, 20 * N)}[kind]


@functools.lru_cache(maxsize=None)
def _demod_ref(N, F, first_bin, cpk, T, precision, offk, ta):
    cp = _cp(N, cpk, T)
    smp = _samples(N, sum(cp) + T * N, precision)
    kw = dict(first_bin=first_bin, timing_advance=ta, offset=_offsets(N, offk))
    ref = O.demodulate(smp, N, cp, F, T, **kw)
    floor = _err(O.demodulate(smp, N, cp, F, T, dtype=np.complex64, **kw), ref) if precision == "f32" else 0.0
    ref.setflags(write=False)
    return ref, floor


def _to_layout(g, layout):
    return g if layout == "planar" else O.to_cgnn(g)


def _from_layout(a, layout):
    return a if layout == "planar" else O.from_cgnn(a)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a writable copy of the cached, read-only input


def _tdt(precision, real=False):
    import torch
    return {("f32", False): torch.complex64, ("f64", False): torch.complex128, ("f32", True): torch.float32,
            ("f64", True): torch.float64}[(precision, real)]


def _modulate(g, N, cp, first_bin, layout, precision, pad=0, pa=None, guarded=True):
    import torch
    from neural_rx_amd.ofdm import OFDMModulator
    T = g.shape[-1]
    L = sum(cp) + T * N + pad
    mod = OFDMModulator(list(cp), fft_size=N, first_bin=first_bin, layout=layout, precision=precision, pa=pa, num_samples=L)
    out, guard = memguard.guarded_out((B, S, L), 0xFF, _tdt(precision))
    got = mod(_dev(_to_layout(g, layout)), out=out)
    torch.cuda.synchronize()
    guard.check("samples")
    return got.cpu().numpy()


def _demodulate(smp, N, cp, F, T, first_bin, layout, precision, offset=0, ta=0):
    import torch
    from neural_rx_amd.ofdm import OFDMDemodulator
    dem = OFDMDemodulator(N, -ta, list(cp), num_subcarriers=F, first_bin=first_bin, layout=layout, precision=precision,
                          offset=list(offset) if not isinstance(offset, int) else offset, num_symbols=T)
    shape = (B, S, F, T) if layout == "planar" else (B, F, T, 2 * S)
    out, guard = memguard.guarded_out(shape, 0xFF, _tdt(precision, real=layout == "cgnn"))
    got = dem(_dev(smp), out=out)
    torch.cuda.synchronize()
    guard.check("grid")
    return _from_layout(got.cpu().numpy(), layout)


# (N, F, first_bin, cp, layout, precision, T)
SHAPES = [
    (64, 64, 0, "nr", "planar", "f32", 14), (64, 48, -1, "nr", "cgnn", "f32", 14), (64, 25, -1, "zero", "planar", "f64", 14),
    (64, 48, 0, "nr", "planar", "f32", 1), (64, 25, 39, "nr", "cgnn", "f64", 1),
    (128, 128, 0, "nr", "cgnn", "f64", 14), (128, 48, -1, "nr", "planar", "f32", 14), (128, 25, 0, "zero", "cgnn", "f32", 14),
    (256, 48, -1, "nr", "planar", "f32", 14), (256, 25, -1, "nr", "cgnn", "f64", 14),
    (512, 512, 0, "nr", "planar", "f32", 14), (512, 48, -1, "zero", "cgnn", "f64", 14), (512, 25, -1, "nr", "planar", "f64", 1),
    (1024, 48, -1, "nr", "cgnn", "f32", 14), (1024, 25, 0, "zero", "planar", "f64", 14),
    (2048, 48, -1, "nr", "planar", "f32", 14), (2048, 25, -1, "nr", "cgnn", "f64", 14),
    (4096, 4096, 0, "nr", "cgnn", "f32", 14), (4096, 48, -1, "nr", "planar", "f64", 14), (4096, 25, 0, "zero", "planar", "f32", 14),
]


@pytest.mark.parametrize("N,F,first_bin,cpk,layout,precision,T", SHAPES)
def test_modulate(N, F, first_bin, cpk, layout, precision, T):
    pad = 0 if F == N else 37           # a tail behind the last symbol, which the call zeroes
    ref, floor = _mod_ref(N, F, first_bin, cpk, T, precision, pad)
    got = _modulate(_grid(N, F, T, precision), N, _cp(N, cpk, T), first_bin, layout, precision, pad)
    assert not np.isnan(got.view(got.real.dtype)).any(), "an element of samples was not written"
    if pad:
        assert not got[..., -pad:].any()
    err, gate = _err(got, ref), _gate(N, precision, floor)
    print(f"modulate N={N} F={F} {precision}: err {err:.3g} floor {floor:.3g} gate {gate:.3g}")
    assert err <= gate


@pytest.mark.parametrize("offk,ta", [("zero", 0), ("mixed", 1), ("far", "cp")])
@pytest.mark.parametrize("N,F,first_bin,cpk,layout,precision,T", SHAPES)
def test_demodulate(N, F, first_bin, cpk, layout, precision, T, offk, ta):
    cp = _cp(N, cpk, T)
    ta = min(cp) if ta == "cp" else min(ta, min(cp))
    ref, floor = _demod_ref(N, F, first_bin, cpk, T, precision, offk, ta)
    smp = _samples(N, sum(cp) + T * N, precision)
    got = _demodulate(smp, N, cp, F, T, first_bin, layout, precision, _offsets(N, offk), ta)
    assert not np.isnan(got.view(got.real.dtype)).any(), "an element of the grid was not written"
    if offk == "far":                   # windows wholly before / behind the row read zeros
        assert not got[:, 0].any() and not got[:, 2].any() and got[:, 1].any()
    err, gate = _err(got, ref), _gate(N, precision, floor)
    print(f"demodulate N={N} F={F} {precision} ta={ta} {offk}: err {err:.3g} floor {floor:.3g} gate {gate:.3g}")
    assert err <= gate


@pytest.mark.parametrize("N,F,first_bin,cpk,layout,precision,T",
                         [s for s in SHAPES if s[6] == 14 and s[1] != s[0] or s[0] == 4096])
def test_round_trip_and_same_bits(N, F, first_bin, cpk, layout, precision, T):
    """demodulate(modulate(g)) = g on the GPU alone, within the gate of one transform; a second call and a call
    per slot give the same bits"""
    g = _grid(N, F, T, precision)
    cp = _cp(N, cpk, T)
    smp = _modulate(g, N, cp, first_bin, layout, precision)
    ta = min(cp)
    back = _demodulate(smp, N, cp, F, T, first_bin, layout, precision, ta=ta)
    ref = g.astype(np.complex128)
    c64 = O.demodulate(O.modulate(g, N, cp, first_bin, dtype=np.complex64), N, cp, F, T, first_bin, ta, dtype=np.complex64)
    floor = _err(c64, ref) if precision == "f32" else 0.0
    err, gate = _err(back, ref), _gate(N, precision, floor)
    print(f"round trip N={N} F={F} {precision}: err {err:.3g} floor {floor:.3g} gate {gate:.3g}")
    assert err <= gate
    assert memguard.same_bits(_modulate(g, N, cp, first_bin, layout, precision), smp)
    assert memguard.same_bits(_demodulate(smp, N, cp, F, T, first_bin, layout, precision, ta=ta), back)


@pytest.mark.parametrize("N,layout,precision", [(64, "cgnn", "f32"), (2048, "planar", "f64")])
def test_batch_split_gives_the_same_bits(N, layout, precision):
    import torch
    from neural_rx_amd.ofdm import OFDMDemodulator, OFDMModulator
    F, cp = 48, _cp(N, "nr")
    g = _dev(_to_layout(_grid(N, F, 14, precision), layout))
    mod = OFDMModulator(cp, fft_size=N, layout=layout, precision=precision)
    dem = OFDMDemodulator(N, -1, cp, num_subcarriers=F, layout=layout, precision=precision, offset=[-2, 0, 3])
    smp = mod(g)
    back = dem(smp)
    host = lambda t: t.cpu().numpy()  # noqa: E731
    for b in range(B):
        part = mod(g[b:b + 1].contiguous())
        assert memguard.same_bits(host(part), host(smp[b:b + 1]))
        assert memguard.same_bits(host(dem(part)), host(back[b:b + 1]))
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,F,precision", [(64, 48, "f32"), (64, 25, "f64"), (512, 48, "f32"), (4096, 48, "f64")])
@pytest.mark.parametrize("rel", [0.5, 1.0, 2.0])
def test_rapp_store(N, F, precision, rel):
    from neural_rx_amd.ofdm import rapp
    asat = rel * float(np.sqrt(F / N))
    ref, floor = _mod_ref(N, F, -1, "nr", 14, precision, 0, asat)
    linear, _ = _mod_ref(N, F, -1, "nr", 14, precision, 0)
    got = _modulate(_grid(N, F, 14, precision), N, _cp(N, "nr"), -1, "planar", precision, pa=rapp(asat, 2.0))
    err, gate = _err(got, ref), _gate(N, precision, floor)
    print(f"rapp N={N} F={F} {precision} asat={rel} rms: err {err:.3g} floor {floor:.3g} gate {gate:.3g}")
    assert err <= gate
    assert np.abs(got).max() < asat and np.abs(linear).max() > asat        # it did compress
