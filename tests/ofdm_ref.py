"""numpy statement of ``nrx_ofdm_modulate`` / ``nrx_ofdm_demodulate`` and of the time-domain transmit stage of
``nrx_generate_slots_td`` (include/nrx.h).  A test helper, not a test.

Grids are complex ``[..., F, T]`` (the PLANAR layout); ``to_cgnn`` / ``from_cgnn`` convert to and from
``[B, F, T, 2S]``.  With N the FFT size, ``bin(f) = (f + first_bin - N/2) mod N`` and both transforms unitary:

    modulate    grid subcarrier f -> bin(f), zeros elsewhere; IDFT; the last cp[t] samples prepended; symbols
                concatenated; the Rapp curve v / (1 + (|v| / A)^(2p))^(1 / (2p)) if asat = A > 0; zeros up to L
    demodulate  the window of symbol t starts at offset + start[t] + cp[t] - timing_advance, zeros outside
                [0, L); DFT; bin k times e^{+j 2 pi k timing_advance / N}; bin(f) -> subcarrier f

The working precision follows ``dtype`` (complex128, or complex64 for the single-precision floor of the GPU
tests: numpy's FFT keeps single precision); the Rapp curve is always evaluated in float64.
``generate`` builds on ``oracle.synth_ref.generate`` the way ``tests.cfo_ref.generate`` does.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np

from oracle import synth_ref as S

T_SLOT = 14


def default_cp(N: int) -> int:
    """9 N / 128: 288 at N = 4096, the normal cyclic prefix of NR"""
    return 9 * N // 128


def cp_list(cp, T: int = T_SLOT) -> list:
    """one int, or T of them"""
    v = [int(c) for c in np.atleast_1d(cp)]
    if len(v) == 1:
        v = v * T
    assert len(v) == T, (len(v), T)
    return v


def resolve_first_bin(first_bin: int, N: int, F: int) -> int:
    return N // 2 - F // 2 if first_bin < 0 else first_bin


def bins(F: int, N: int, first_bin: int = -1) -> np.ndarray:
    """bin(f) of every grid subcarrier, unshifted 0..N-1"""
    return np.mod(np.arange(F) + resolve_first_bin(first_bin, N, F) - N // 2, N)


def starts(cp: Sequence[int], N: int) -> np.ndarray:
    """first sample of every symbol, and the total behind the last"""
    return np.concatenate([[0], np.cumsum(np.asarray(cp) + N)])


def rapp(v: np.ndarray, asat: float, p: float) -> np.ndarray:
    """float64 arithmetic, the result in v's dtype; asat <= 0: the identity"""
    if not asat > 0:
        return v
    z = v.astype(np.complex128)
    g = (1.0 + ((z.real ** 2 + z.imag ** 2) / (asat * asat)) ** p) ** (-0.5 / p)
    return (z * g).astype(v.dtype)


def modulate(grid: np.ndarray, N: int, cp, first_bin: int = -1, L: Optional[int] = None, asat: float = 0.0,
             p: float = 2.0, dtype=np.complex128) -> np.ndarray:
    """grid [..., F, T] -> samples [..., L]"""
    grid = np.asarray(grid).astype(dtype)
    F, T = grid.shape[-2:]
    cp = cp_list(cp, T)
    st = starts(cp, N)
    L = int(st[-1]) if L is None else L
    assert L >= st[-1]
    X = np.zeros(grid.shape[:-2] + (N, T), dtype)
    X[..., bins(F, N, first_bin), :] = grid
    x = (np.fft.ifft(X, axis=-2) * np.asarray(np.sqrt(N), X.real.dtype)).astype(dtype)      # unitary
    out = np.zeros(grid.shape[:-2] + (L,), dtype)
    for t in range(T):
        out[..., st[t]:st[t] + cp[t]] = x[..., N - cp[t]:, t]
        out[..., st[t] + cp[t]:st[t + 1]] = x[..., :, t]
    out[..., :st[-1]] = rapp(out[..., :st[-1]], asat, p)
    return out


def demodulate(samples: np.ndarray, N: int, cp, F: int, T: int = T_SLOT, first_bin: int = -1,
               timing_advance: int = 0, offset=0, dtype=np.complex128) -> np.ndarray:
    """samples [..., S, L] -> grid [..., S, F, T]; ``offset``: one int or one per stream (axis -2)"""
    samples = np.asarray(samples).astype(dtype)
    S_, L = samples.shape[-2:]
    cp = cp_list(cp, T)
    st = starts(cp, N)
    off = [int(o) for o in np.atleast_1d(offset)]
    off = off * S_ if len(off) == 1 else off
    assert len(off) == S_ and 0 <= timing_advance <= min(cp)
    w = np.zeros(samples.shape[:-1] + (N, T), dtype)
    for s in range(S_):
        for t in range(T):
            w0 = off[s] + int(st[t]) + cp[t] - timing_advance
            lo, hi = max(w0, 0), min(w0 + N, L)
            if hi > lo:
                w[..., s, lo - w0:hi - w0, t] = samples[..., s, lo:hi]
    X = (np.fft.fft(w, axis=-2) / np.asarray(np.sqrt(N), w.real.dtype)).astype(dtype)
    ramp = np.exp(2j * np.pi * (np.arange(N) * timing_advance % N) / N).astype(dtype)
    X = X * ramp[:, None]
    return X[..., bins(F, N, first_bin), :]


def to_cgnn(grid: np.ndarray) -> np.ndarray:
    """[B, S, F, T] complex -> [B, F, T, 2S] real, Re s0..s(S-1) then Im"""
    g = np.moveaxis(grid, 1, -1)
    return np.ascontiguousarray(np.concatenate([g.real, g.imag], axis=-1))


def from_cgnn(y: np.ndarray) -> np.ndarray:
    """[B, F, T, 2S] real -> [B, S, F, T] complex"""
    S_ = y.shape[-1] // 2
    return np.ascontiguousarray(np.moveaxis(y[..., :S_] + 1j * y[..., S_:], -1, 1))


def delay_ramp(F: int, N: int, delay: int, first_bin: int = -1) -> np.ndarray:
    """e^{-j 2 pi delay k_f / N}, k_f = f + first_bin - N/2 signed: what a delay inside the cyclic prefix does"""
    kf = np.arange(F) + resolve_first_bin(first_bin, N, F) - N // 2
    return np.exp(-2j * np.pi * (delay * kf % N) / N)


def pa_asat(F: int, N: int, ibo_db: float) -> float:
    """the generator's saturation amplitude: ibo_db over the nominal rms sample amplitude sqrt(F / N)"""
    return float(np.sqrt(F / N) * 10.0 ** (ibo_db / 20.0))


def tx_stage(x: np.ndarray, N: int, cp, delay: Sequence[int], first_bin: int = -1, pa_ibo_db: Optional[float] = None,
             pa_smoothness: float = 2.0) -> np.ndarray:
    """x [B, U, F, 14] -> x' = demodulate(impair(modulate(x))), float64"""
    F, T = x.shape[-2:]
    asat = pa_asat(F, N, pa_ibo_db) if pa_ibo_db is not None else 0.0
    smp = modulate(x, N, cp, first_bin, asat=asat, p=pa_smoothness)
    return demodulate(smp, N, cp, F, T, first_bin, 0, [-int(d) for d in delay])


@dataclasses.dataclass
class TdOut:
    y: np.ndarray           # [B, F, T, 2A] f32
    h_hat: np.ndarray       # [B, U, F, T, 2A] f32
    h: np.ndarray           # [B, U, F, T, 2A] f32
    x_out: np.ndarray       # [B, U, F, T] c128
    base: S.GenOut


def _cplx(z: np.ndarray) -> np.ndarray:
    A = z.shape[-1] // 2
    return z[..., :A].astype(np.float64) + 1j * z[..., A:].astype(np.float64)


def _chan(z: np.ndarray) -> np.ndarray:
    return np.concatenate([z.real, z.imag], axis=-1).astype(np.float32)


def generate(s: S.GenSpec, N: int, cp, delay: Sequence[int], first_bin: int = -1, pa_ibo_db: Optional[float] = None,
             pa_smoothness: float = 2.0, h_with_delay: bool = False, base: Optional[S.GenOut] = None) -> TdOut:
    """the generator with the stage: y' = y_c + sum_u h_u (x'_u - x_u) on the generator's own h (f32, whose
    rounding contributes at most 2^-24 |h| |x' - x| to y'), the LS division by the clean pilot"""
    o = base if base is not None else S.generate(s)
    B, U, F, A, T = s.batch, s.num_tx, s.num_subcarriers, s.num_rx_ant, s.num_symbols
    xp = tx_stage(o.x, N, cp, delay, first_bin, pa_ibo_db, pa_smoothness)
    h = _cplx(o.h)
    y_c = np.moveaxis(o.y_c, 1, -1).copy() + (h * (xp - o.x)[..., None]).sum(1)
    y = _chan(y_c)
    yr = _cplx(y)
    h_hat = np.zeros((B, U, F, T, A), np.complex128)
    h_out = h.copy()
    for u in range(U):
        fp, tp = S.nearest_pilot(F, s.dmrs_symbols, s.cdm_group[u], T)
        xpil = o.x[:, u, fp, tp]
        safe = np.where(xpil != 0, xpil, 1.0)
        h_hat[:, u] = np.where((xpil != 0)[..., None], yr[:, fp, tp, :] / safe[..., None], 0)
        if h_with_delay:
            h_out[:, u] *= delay_ramp(F, N, int(delay[u]), first_bin)[None, :, None, None]
    return TdOut(y=y, h_hat=_chan(h_hat), h=_chan(h_out) if h_with_delay else o.h, x_out=xp, base=o)
