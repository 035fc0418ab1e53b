"""numpy float64 statement of the carrier frequency offset of ``nrx_generate_slots_cfo`` and of
``nrx_cfo_estimate`` / ``nrx_cfo_rotate`` (include/nrx.h).  A test helper, not a test.

The impairment, per (slot, user) with eps the offset in subcarrier spacings, N the FFT size and
kappa = ``oracle.synth_ref.CP_FACTOR``:

    x'[k, t] = e^{j theta_t} sum_{m < F} c[m - k] x[m, t]
    c[d]     = D_N(d + eps),  D_N(v) = e^{j pi (N - 1) v / N} sin(pi v) / (N sin(pi v / N)),
               D_N(v) = 1 where v / N is an integer
    theta_t  = 2 pi eps (kappa t + (kappa - 1))

``generate`` builds on ``oracle.synth_ref.generate`` (or ``tests.synth_chan_ref.generate``): its
``x``, ``y_c`` and ``h``, and its ``draw`` / ``uniform`` for eps:  y' = y_c + sum_u h_u (x'_u - x_u).
``h`` is the f32 ``GenOut.h``, whose rounding contributes at most 2^-24 |h| |x' - x| to y'.
``ofdm_chain`` is the independent statement the closed form is tested against: IFFT, rotation of the
time samples, FFT.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np

from oracle import synth_ref as S

STREAM_CFO = 6
KAPPA = S.CP_FACTOR
REF_NEAREST_DMRS, REF_ZERO = 0, 1


def lags(d, eps: float, N: int) -> np.ndarray:
    """c[d] = D_N(d + eps) for integer lags d.  With eps = n + r, n = rint(eps): sin(pi (d + eps)) =
    (-1)^(d + n) sin(pi r) and e^{j pi (d + eps)} = (-1)^(d + n) e^{j pi r}, so
    c[d] = K (cot(phi) - j), K = e^{j pi r} sin(pi r) / N, phi = pi (q + r) / N with q = (d + n) mod N in
    (-N/2, N/2]; r = 0 is the exact shift [q == 0]."""
    d = np.asarray(d, np.int64)
    n = float(np.rint(eps))
    r = float(eps) - n
    q = np.mod(d + int(n), N).astype(np.float64)
    q = np.where(2 * q > N, q - N, q)
    if r == 0.0:
        return (q == 0).astype(np.complex128)
    K = np.exp(1j * np.pi * r) * np.sin(np.pi * r) / N
    phi = np.pi * ((q + r) / N)
    return K * (np.cos(phi) / np.sin(phi) - 1j)


def toeplitz(F: int, eps: float, N: int) -> np.ndarray:
    """C [F, F] with C[k, m] = c[m - k]"""
    k = np.arange(F)
    return lags(k[None, :] - k[:, None], eps, N)


def theta(eps, T: int = 14) -> np.ndarray:
    """theta_t [..., T]"""
    return 2.0 * np.pi * (np.asarray(eps, np.float64)[..., None] * (KAPPA * np.arange(T) + (KAPPA - 1.0)))


def apply(x: np.ndarray, eps: float, N: int) -> np.ndarray:
    """x [F, T] -> x' [F, T]"""
    F, T = x.shape
    return np.exp(1j * theta(eps, T))[None, :] * (toeplitz(F, eps, N) @ x)


def ofdm_chain(x: np.ndarray, eps: float, N: int) -> np.ndarray:
    """The same map by its definition: the F subcarriers on bins 0..F-1 of an N-point IFFT, sample n
    of symbol t (n = 0 the first one behind a cyclic prefix of (kappa - 1) N samples, symbols kappa N
    samples apart) rotated by e^{j 2 pi (eps / N) (n0_t + n)}, FFT, bins 0..F-1."""
    F, T = x.shape
    X = np.zeros((N, T), np.complex128)
    X[:F] = x
    s = np.fft.ifft(X, axis=0)
    n0 = KAPPA * N * np.arange(T) + (KAPPA - 1.0) * N
    rot = np.exp(2j * np.pi * (eps / N) * (n0[None, :] + np.arange(N)[:, None]))
    return np.fft.fft(s * rot, axis=0)[:F]


def draw_eps(s: S.GenSpec, cfo_hz: Sequence[float], constant: bool) -> np.ndarray:
    """eps [B, U]"""
    B, U = s.batch, s.num_tx
    emax = np.array([float(cfo_hz[u]) / s.subcarrier_spacing for u in range(U)])
    if constant:
        return np.broadcast_to(emax, (B, U)).copy()
    slots = s.slot_offset + np.arange(B, dtype=np.int64)
    w = S.draw(s.seed, slots[:, None], STREAM_CFO, np.arange(U)[None, :])[0]
    return emax[None, :] * (2.0 * S.uniform(w) - 1.0)


@dataclasses.dataclass
class CfoOut:
    y: np.ndarray           # [B, F, T, 2A] f32
    h_hat: np.ndarray       # [B, U, F, T, 2A] f32
    h: np.ndarray           # [B, U, F, T, 2A] f32
    eps: np.ndarray         # [B, U] f64
    base: S.GenOut          # the generator without the offset


def _cplx(z: np.ndarray) -> np.ndarray:
    A = z.shape[-1] // 2
    return z[..., :A].astype(np.float64) + 1j * z[..., A:].astype(np.float64)


def _chan(z: np.ndarray) -> np.ndarray:
    return np.concatenate([z.real, z.imag], axis=-1).astype(np.float32)


def generate(s: S.GenSpec, cfo_hz: Sequence[float], constant: bool = False, fft_size: int = 0,
             h_with_phase: bool = False, base: Optional[S.GenOut] = None) -> CfoOut:
    """``base``: the output of the generator without the offset for ``s`` (default
    ``oracle.synth_ref.generate(s)``; ``tests.synth_chan_ref.generate`` for per-user channels)."""
    o = base if base is not None else S.generate(s)
    B, U, F, A, T = s.batch, s.num_tx, s.num_subcarriers, s.num_rx_ant, s.num_symbols
    N = fft_size or F
    eps = draw_eps(s, cfo_hz, constant)
    h = _cplx(o.h)                                               # [B, U, F, T, A]
    y_c = np.moveaxis(o.y_c, 1, -1).copy()                       # [B, F, T, A]
    h_out = h.copy()
    for b in range(B):
        for u in range(U):
            xp = apply(o.x[b, u], eps[b, u], N)
            y_c[b] += h[b, u] * (xp - o.x[b, u])[:, :, None]
            if h_with_phase:
                h_out[b, u] *= (np.exp(1j * theta(eps[b, u], T)) * lags(0, eps[b, u], N))[None, :, None]
    y = _chan(y_c)
    yr = _cplx(y)
    h_hat = np.zeros((B, U, F, T, A), np.complex128)
    for u in range(U):
        fp, tp = S.nearest_pilot(F, s.dmrs_symbols, s.cdm_group[u], T)
        xpil = o.x[:, u, fp, tp]
        safe = np.where(xpil != 0, xpil, 1.0)
        h_hat[:, u] = np.where((xpil != 0)[..., None], yr[:, fp, tp, :] / safe[..., None], 0)
    return CfoOut(y=y, h_hat=_chan(h_hat), h=_chan(h_out) if h_with_phase else o.h, eps=eps, base=o)


def aerial_pilots(h_hat: np.ndarray, dmrs_symbols: Sequence[int], cdm_group: Sequence[int]):
    """(h_ls_real, h_ls_imag) [B, Npil, U, A] of include/nrx.h nrx_aerial_io from h_hat: pilot
    p = (k * nprb + prb) * 6 + j of user u is subcarrier prb * 12 + cdm + 2 j of DMRS symbol k"""
    B, U, F, T, A2 = h_hat.shape
    A, nprb = A2 // 2, F // 12
    out = np.zeros((2, B, len(dmrs_symbols) * nprb * 6, U, A), np.float32)
    for u in range(U):
        for k, t in enumerate(dmrs_symbols):
            for prb in range(nprb):
                for j in range(6):
                    v = h_hat[:, u, prb * 12 + cdm_group[u] + 2 * j, t]
                    out[0][:, (k * nprb + prb) * 6 + j, u] = v[:, :A]
                    out[1][:, (k * nprb + prb) * 6 + j, u] = v[:, A:]
    return out[0], out[1]


def estimate(h_hat: np.ndarray, active: np.ndarray, dmrs_symbols: Sequence[int],
             cdm_group: Sequence[int]) -> np.ndarray:
    """eps_hat [B, U] (nrx_cfo_estimate)"""
    B, U, F, T, _ = h_hat.shape
    hc = _cplx(h_hat)
    out = np.zeros((B, U))
    D = list(dmrs_symbols)
    if len(D) < 2:
        return out
    g = min(b - a for a, b in zip(D, D[1:]))
    for u in range(U):
        p = np.arange(cdm_group[u], F, 2)
        r = np.zeros(B, np.complex128)
        for a, b in zip(D, D[1:]):
            if b - a == g:
                r += (hc[:, u, p, b, :] * hc[:, u, p, a, :].conj()).sum((1, 2))
        out[:, u] = np.where((r != 0) & (active[:, u] > 0), np.angle(r) / (2.0 * np.pi * KAPPA * g), 0.0)
    return out


def nearest_symbol(dmrs_symbols: Sequence[int], T: int = 14) -> np.ndarray:
    """t_ref [T]: the first listed DMRS symbol nearest t (oracle.synth_ref.nearest_pilot's rule)"""
    D = np.array(list(dmrs_symbols))
    return D[np.abs(np.arange(T)[:, None] - D[None, :]).argmin(-1)]


def rotate(h: np.ndarray, eps: np.ndarray, dmrs_symbols: Sequence[int], ref_mode: int, sign: int) -> np.ndarray:
    """h [B, U, F, T, 2A] f32 -> f32 (nrx_cfo_rotate)"""
    T = h.shape[3]
    tref = nearest_symbol(dmrs_symbols, T) if ref_mode == REF_NEAREST_DMRS else np.zeros(T, np.int64)
    ph = sign * 2.0 * np.pi * KAPPA * eps[:, :, None] * (np.arange(T) - tref)[None, None, :]     # [B, U, T]
    return _chan(_cplx(h) * np.exp(1j * ph)[:, :, None, :, None])


def nmse(h_est: np.ndarray, h_true: np.ndarray, active: np.ndarray) -> float:
    """sum |h_est - h_true|^2 / sum |h_true|^2 over the active (slot, user) pairs"""
    m = (active > 0)[:, :, None, None, None]
    e = (h_est.astype(np.float64) - h_true.astype(np.float64)) ** 2
    return float((e * m).sum() / ((h_true.astype(np.float64) ** 2) * m).sum())
