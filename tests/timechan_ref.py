"""numpy statement of the time-domain channel ``nrx_time_channel`` and of the slot generator with it,
``nrx_generate_slots_tc`` (include/nrx.h).  A test helper, not a test.

With fs the sample rate, sinc(0) = 1, sinc(v) = sin(pi v) / (pi v) and x read as zero outside [0, Ls):

    r[b,a,n] = sum_u sum_l g[b,u,a,l](n) v[b,u,l](n)
    g(n)     = sum_{s<NS} g0[b,u,a,l,s] exp(j 2 pi fd[b,u,a,l,s] (n - n0) / fs)
    v(n)     = sum_{l'=l_min..l_max} sinc(l' - tau[b,u,l] fs) x[b,u,n - l']

and with an antenna mix M, r'[a] = sum_a' M[a][a'] r[a'] (a' ascending).  The sinc is plainly truncated: no
window, no re-normalisation.  ``time_channel`` takes the working precision as ``real`` (float64, or longdouble
for the floor of the GPU tests: the error of the float64 statement against the same statement in longdouble).

``generate`` builds the generator's slot on ``oracle.synth_ref`` and ``tests.synth_chan_ref``: tau, g0 (sqrt(pdp)
folded in) and fd are the built-in channel's draws, n0 = cp[0], each path carries the phase
exp(+j 2 pi (first_bin - N/2) scs tau_l), fs = N scs; the samples are ``ofdm_ref.modulate(x)``, the A received
streams are demodulated with ``timing_advance = ta``, the generator's grid noise (same draws) is added after
demodulation, LS divides by the clean pilot, and h is the ISI-free diagonal of the effective channel

    h[b,u,f,t,a] = sum_l' hbar_t[l'] exp(-j 2 pi k_f l' / N),    k_f = f + first_bin - N/2
    hbar_t[l']   = (1/N) sum_{m<N} h_{u,a}[w_t + m, l'],         w_t = start[t] + cp[t] - ta
    h_{u,a}[n,l'] = sum_l g(n) sinc(l' - tau_l fs)

exact when l_max <= cp - ta and ta >= -l_min, the dominant term otherwise.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Sequence

import numpy as np

from oracle import synth_ref as S
from tests import ofdm_ref as O
from tests import synth_chan_ref as C

PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def _pi(real):
    return PI_LD if real is np.longdouble else real(np.pi)


def _cplx(real):
    return np.clongdouble if real is np.longdouble else np.complex128


def sinc(v: np.ndarray, real=np.float64) -> np.ndarray:
    v = np.asarray(v, real)
    safe = np.where(v == 0, real(1), v)
    return np.where(v == 0, real(1), np.sin(_pi(real) * safe) / (_pi(real) * safe))


def fir_taps(tau: np.ndarray, fs: float, l_min: int, l_max: int, real=np.float64) -> np.ndarray:
    """sinc(l' - tau fs), [..., span]"""
    lp = np.arange(l_min, l_max + 1).astype(real)
    return sinc(lp - (np.asarray(tau, real) * real(fs))[..., None], real)


def gains(g0: np.ndarray, fd: np.ndarray, fs: float, n0: int, n: np.ndarray, real=np.float64) -> np.ndarray:
    """g [B, U, A, L, len(n)]: the sum of sinusoids at the samples ``n``, s ascending"""
    g0 = np.asarray(g0, _cplx(real))
    fd = np.asarray(fd, real)
    tn = (np.asarray(n) - n0).astype(real) / real(fs)
    g = np.zeros(g0.shape[:-1] + (len(tn),), _cplx(real))
    for s in range(g0.shape[-1]):
        ph = real(2) * _pi(real) * (fd[..., s, None] * tn)
        g += g0[..., s, None] * (np.cos(ph) + 1j * np.sin(ph))
    return g


def time_channel(x, tau, g0, fd, fs: float, n0: int, l_min: int, l_max: int, rx_mix=None,
                 real=np.float64) -> np.ndarray:
    """x [B, U, Ls], tau [B, U, L], g0 / fd [B, U, A, L, NS] -> r [B, A, Ls]"""
    x = np.asarray(x, _cplx(real))
    B, U, Ls = x.shape
    A, L = g0.shape[2], g0.shape[3]
    c = fir_taps(tau, fs, l_min, l_max, real)                            # [B, U, L, span]
    v = np.zeros((B, U, L, Ls), _cplx(real))
    for j, lp in enumerate(range(l_min, l_max + 1)):                     # v += c x[n - l'], l' ascending
        lo, hi = max(lp, 0), min(Ls + lp, Ls)                            # n in [lo, hi): 0 <= n - l' < Ls
        if hi > lo:
            v[..., lo:hi] += c[..., j, None] * x[:, :, None, lo - lp:hi - lp]
    g = gains(g0, fd, fs, n0, np.arange(Ls), real)                       # [B, U, A, L, Ls]
    r = np.zeros((B, A, Ls), _cplx(real))
    for u in range(U):
        for l in range(L):
            r += g[:, u, :, l] * v[:, u, None, l]
    if rx_mix is not None:
        M = np.asarray(rx_mix, _cplx(real))
        mixed = np.zeros_like(r)
        for a2 in range(A):
            mixed += M[None, :, a2, None] * r[:, a2:a2 + 1]
        r = mixed
    return r


def effective_h(tau, g0, fd, N: int, cp, F: int, fs: float, n0: int, l_min: int, l_max: int, ta: int,
                first_bin: int = -1, rx_mix=None) -> np.ndarray:
    """the ISI-free diagonal h [B, U, A, F, T] complex128 (module docstring); the mix acts on the mean taps"""
    cp = O.cp_list(cp)
    st = O.starts(cp, N)
    T = len(cp)
    A = g0.shape[2]
    gbar = []
    for t in range(T):
        w = int(st[t]) + cp[t] - ta
        gbar.append(gains(g0, fd, fs, n0, np.arange(w, w + N)).mean(-1))
    gbar = np.stack(gbar, -1)                                            # [B, U, A, L, T]
    if rx_mix is not None:
        M = np.asarray(rx_mix, np.complex128)
        mixed = np.zeros_like(gbar)
        for a2 in range(A):
            mixed += M[None, None, :, a2, None, None] * gbar[:, :, a2:a2 + 1]
        gbar = mixed
    c = fir_taps(tau, fs, l_min, l_max)                                  # [B, U, L, span]
    kf = np.arange(F) + O.resolve_first_bin(first_bin, N, F) - N // 2
    lp = np.arange(l_min, l_max + 1)
    ramp = np.exp(-2j * np.pi * (np.outer(lp, kf) % N) / N)               # [span, F]
    E = np.einsum("bulj,jf->bulf", c, ramp)
    return np.einsum("bualt,bulf->buaft", gbar, E)


def resolve_l_max(l_max: int, max_delay_s: Sequence[float], fs: float) -> int:
    return l_max if l_max >= 0 else int(math.ceil(max(max_delay_s) * fs)) + 6


def channel_draws(s: S.GenSpec, N: int, first_bin: int = -1, user_profiles: Optional[Sequence] = None):
    """(tau [B,U,L], g0 [B,U,A,L,NS] with sqrt(pdp) and the grid-reference phase folded in, fd [B,U,A,L,NS]):
    the draws of ``tests.synth_chan_ref.generate``, unsummed"""
    B, U, A, L, NS = s.batch, s.num_tx, s.num_rx_ant, s.num_taps, s.num_sinusoids
    if user_profiles is None:
        user_profiles = [(s.max_delay_s, s.max_doppler_hz)] * U
    max_delay = np.array([p[0] for p in user_profiles], np.float64)
    max_doppler = np.array([p[1] for p in user_profiles], np.float64)
    slots = s.slot_offset + np.arange(B, dtype=np.int64)
    didx = np.arange(U)[:, None] * L + np.arange(L)[None, :]
    dw = S.draw(s.seed, slots[:, None, None], S.STREAM_DELAY, didx[None])[0]
    tau = np.sort(S.uniform(dw) * max_delay[None, :, None], axis=-1)
    tau[..., 0] = 0.0
    pdp = np.exp(-tau / (max_delay[None, :, None] / S.PDP_DECAY + 1e-12))
    pdp = pdp / pdp.sum(-1, keepdims=True)
    tidx = (((np.arange(U)[:, None, None, None] * A + np.arange(A)[None, :, None, None]) * L
             + np.arange(L)[None, None, :, None]) * NS + np.arange(NS)[None, None, None, :])
    t0, t1, t2, _ = S.draw(s.seed, slots[:, None, None, None, None], S.STREAM_TAP, tidx[None])
    nre, nim = S.box_muller(t0, t1)
    g0 = (nre + 1j * nim) / np.sqrt(2.0 * NS) * np.sqrt(pdp)[:, :, None, :, None]
    fb = O.resolve_first_bin(first_bin, N, s.num_subcarriers)
    ph = 2.0 * np.pi * (((fb - N // 2) * s.subcarrier_spacing) * tau)
    g0 = g0 * (np.cos(ph) + 1j * np.sin(ph))[:, :, None, :, None]
    fd = max_doppler[None, :, None, None, None] * np.cos(2.0 * np.pi * S.uniform(t2))
    return tau, g0, fd


def noise(s: S.GenSpec) -> np.ndarray:
    """the generator's grid noise [B, A, F, T] complex128"""
    B, F, A, T = s.batch, s.num_subcarriers, s.num_rx_ant, s.num_symbols
    slots = s.slot_offset + np.arange(B, dtype=np.int64)
    nidx = (np.arange(A)[:, None, None] * F + np.arange(F)[None, :, None]) * T + np.arange(T)[None, None, :]
    n0, n1, _, _ = S.draw(s.seed, slots[:, None, None, None], S.STREAM_NOISE, nidx[None])
    zr, zi = S.box_muller(n0, n1)
    return np.sqrt(s.no / 2.0) * (zr + 1j * zi)


@dataclasses.dataclass
class TcOut:
    y: np.ndarray           # [B, F, T, 2A] f32
    h_hat: np.ndarray       # [B, U, F, T, 2A] f32 (nearest own pilot of the uncovered ports)
    h: np.ndarray           # [B, U, F, T, 2A] f32
    r: np.ndarray           # [B, A, Ls] c128, noise-free
    xs: np.ndarray          # [B, U, Ls] c128, the transmitted samples
    y_free: np.ndarray      # [B, A, F, T] c128, the noise-free demodulated grid
    h_c: np.ndarray         # [B, U, A, F, T] c128
    base: S.GenOut


def _chan(z: np.ndarray) -> np.ndarray:     # [..., A, F, T] -> [..., F, T, 2A] f32
    z = np.moveaxis(z, -3, -1)
    return np.concatenate([z.real, z.imag], axis=-1).astype(np.float32)


def generate(s: S.GenSpec, N: int, cp, l_min: int = -6, l_max: int = -1, ta: int = 0, first_bin: int = -1,
             user_profiles: Optional[Sequence] = None, rx_mix: Optional[np.ndarray] = None,
             base: Optional[S.GenOut] = None, x: Optional[np.ndarray] = None) -> TcOut:
    """``base``: the plain run (bits, mcs, active, x), computed when missing; ``x``: a transmit grid in place of
    base.x (cover-coded pilots)"""
    o = base if base is not None else C.generate(s, user_profiles, rx_mix)
    B, U, F, A, T = s.batch, s.num_tx, s.num_subcarriers, s.num_rx_ant, s.num_symbols
    x = o.x if x is None else x
    cp = O.cp_list(cp)
    fs = N * s.subcarrier_spacing
    delays = [p[0] for p in user_profiles] if user_profiles is not None else [s.max_delay_s]
    l_max = resolve_l_max(l_max, delays, fs)
    tau, g0, fd = channel_draws(s, N, first_bin, user_profiles)
    xs = O.modulate(x, N, cp, first_bin)
    r = time_channel(xs, tau, g0, fd, fs, cp[0], l_min, l_max, rx_mix)
    y_free = O.demodulate(r, N, cp, F, T, first_bin, ta)                 # [B, A, F, T]
    h_c = effective_h(tau, g0, fd, N, cp, F, fs, cp[0], l_min, l_max, ta, first_bin, rx_mix)
    y = _chan(y_free + noise(s))
    yr = y[..., :A].astype(np.float64) + 1j * y[..., A:].astype(np.float64)
    h_hat = np.zeros((B, U, F, T, A), np.complex128)
    for u in range(U):
        fp, tp = S.nearest_pilot(F, s.dmrs_symbols, s.cdm_group[u], T)
        xp = x[:, u, fp, tp]
        safe = np.where(xp != 0, xp, 1.0)
        h_hat[:, u] = np.where((xp != 0)[..., None], yr[:, fp, tp, :] / safe[..., None], 0)
    h_hat = np.concatenate([h_hat.real, h_hat.imag], axis=-1).astype(np.float32)
    return TcOut(y=y, h_hat=h_hat, h=_chan(h_c), r=r, xs=xs, y_free=y_free, h_c=h_c, base=o)
