"""numpy float64 statement of ``nrx_generate_slots_cir`` and ``nrx_generate_taps`` (include/nrx.h): the slot
generator of ``oracle/synth_ref.py`` on a caller-supplied set of channel impulse responses.  A test helper,
not a test.

Dataset.  ``a [E, A, L, Ta]`` complex (float32 parts on the device), ``tau [E, L]`` seconds; Ta is 1 or 14.

Example of (slot b, user u), by ``select``:

    0   e = index[b, u]; a value outside 0..E-1 gives that user a zero channel
    1   e = w mod E, w = word 0 of draw(seed, slot_offset + b, stream 8, element u)
    2   n = E // U, e = U (w mod n) + u          (user u stays on the examples that are u modulo U)

Channel, with g_l(t) = a[e, a, l, 0 if Ta == 1 else t]:

    H_u[a, f, t] = sum_{l < L} g_l(t) exp(-j 2 pi ((f + f_offset) subcarrier_spacing) tau[e, l])

summed with l ascending.  ``normalize``: c[b, u] = mean over (a, f, t) of |H_u|^2, H_u <- H_u / sqrt(c), zeros
where c = 0.  Then y = sum_u H_u x_u + noise with the transmitted grid ``GenOut.x`` of ``oracle.synth_ref.generate``
and its noise draws (stream 5, element (a F + f) 14 + t), and the LS estimate at the nearest own pilot of the
rounded y.  ``bits``, ``mcs`` and ``active`` are those of ``oracle.synth_ref.generate``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from oracle import synth_ref as S

STREAM_CIR = 8
SELECT_INDEX, SELECT_RANDOM, SELECT_TRAJECTORY = 0, 1, 2


def select_examples(s: S.GenSpec, num_examples: int, select: int, index: Optional[np.ndarray] = None) -> np.ndarray:
    """e [B, U] int64, -1 where the user has a zero channel"""
    B, U, E = s.batch, s.num_tx, int(num_examples)
    if select == SELECT_INDEX:
        e = np.asarray(index, np.int64).reshape(B, U)
    else:
        slots = s.slot_offset + np.arange(B, dtype=np.int64)
        w = S.draw(s.seed, slots[:, None], STREAM_CIR, np.arange(U)[None, :])[0].astype(np.int64)
        if select == SELECT_RANDOM:
            e = w % E
        elif select == SELECT_TRAJECTORY:
            n = E // U
            assert n >= 1
            e = U * (w % n) + np.arange(U)[None, :]
        else:
            raise ValueError(select)
    return np.where((e >= 0) & (e < E), e, -1)


def channel(a: np.ndarray, tau: np.ndarray, e: np.ndarray, num_subcarriers: int, subcarrier_spacing: float,
            f_offset: float = 0.0, normalize: bool = False, num_symbols: int = 14) -> np.ndarray:
    """H [B, U, A, F, T] complex128 of the examples e [B, U]"""
    a = np.asarray(a, np.complex128)
    tau = np.asarray(tau, np.float64)
    E, A, L, Ta = a.shape
    assert tau.shape == (E, L) and Ta in (1, num_symbols)
    B, U = e.shape
    F, T = num_subcarriers, num_symbols
    f = np.arange(F, dtype=np.float64)
    H = np.zeros((B, U, A, F, T), np.complex128)
    for b in range(B):
        for u in range(U):
            if e[b, u] < 0:
                continue
            g = np.broadcast_to(a[e[b, u]], (A, L, T))
            for l in range(L):                                               # l ascending
                fa = 2.0 * np.pi * (((f + f_offset) * subcarrier_spacing) * tau[e[b, u], l])
                H[b, u] += g[:, l, None, :] * (np.cos(fa) - 1j * np.sin(fa))[None, :, None]
            if normalize:
                c = np.mean(np.abs(H[b, u]) ** 2)
                H[b, u] = H[b, u] / np.sqrt(c) if c > 0 else 0.0
    return H


def noise(s: S.GenSpec) -> np.ndarray:
    """the generator's AWGN [B, A, F, T] complex128"""
    B, F, A, T = s.batch, s.num_subcarriers, s.num_rx_ant, s.num_symbols
    slots = s.slot_offset + np.arange(B, dtype=np.int64)
    nidx = (np.arange(A)[:, None, None] * F + np.arange(F)[None, :, None]) * T + np.arange(T)[None, None, :]
    n0, n1, _, _ = S.draw(s.seed, slots[:, None, None, None], S.STREAM_NOISE, nidx[None])
    zr, zi = S.box_muller(n0, n1)
    return np.sqrt(s.no / 2.0) * (zr + 1j * zi)


def to_ch(z: np.ndarray) -> np.ndarray:
    """[..., A, F, T] complex -> [..., F, T, 2A] f32"""
    z = np.moveaxis(z, -3, -1)
    return np.concatenate([z.real, z.imag], axis=-1).astype(np.float32)


def ls_nearest(s: S.GenSpec, y: np.ndarray, x: np.ndarray) -> np.ndarray:
    """h_hat [B, U, F, T, 2A] f32: LS at the nearest own pilot of the rounded y (oracle.synth_ref.generate)"""
    B, U, F, A, T = s.batch, s.num_tx, s.num_subcarriers, s.num_rx_ant, s.num_symbols
    yr = y[..., :A].astype(np.float64) + 1j * y[..., A:].astype(np.float64)
    h_hat = np.zeros((B, U, F, T, A), np.complex128)
    for u in range(U):
        fp, tp = S.nearest_pilot(F, s.dmrs_symbols, s.cdm_group[u], T)
        xp = x[:, u, fp, tp]
        safe = np.where(xp != 0, xp, 1.0)
        h_hat[:, u] = np.where((xp != 0)[..., None], yr[:, fp, tp, :] / safe[..., None], 0)
    return np.concatenate([h_hat.real, h_hat.imag], axis=-1).astype(np.float32)


def generate(s: S.GenSpec, a: np.ndarray, tau: np.ndarray, select: int = SELECT_RANDOM,
             index: Optional[np.ndarray] = None, normalize: bool = False, f_offset: float = 0.0,
             base: Optional[S.GenOut] = None):
    """(GenOut on the replayed channel, H [B, U, A, F, T] complex128 unrounded, e [B, U]).  ``base``: the
    built-in run of ``s`` (default ``oracle.synth_ref.generate(s)``), whose x, bits, mcs and active are kept."""
    o = base if base is not None else S.generate(s)
    assert np.asarray(a).shape[1] == s.num_rx_ant
    e = select_examples(s, np.asarray(a).shape[0], select, index)
    H = channel(a, tau, e, s.num_subcarriers, s.subcarrier_spacing, f_offset, normalize, s.num_symbols)
    y_c = np.einsum("buaft,buft->baft", H, o.x) + noise(s)
    y = to_ch(y_c)
    out = S.GenOut(y=y, h_hat=ls_nearest(s, y, o.x), h=to_ch(H), active=o.active, mcs=o.mcs, bits=o.bits, x=o.x,
                   y_c=y_c)
    return out, H, e


def oracle_taps(s: S.GenSpec):
    """(gt [B, U, A, L, T] complex128, tau [B, U, L] float64): the finished taps and delays of
    ``oracle.synth_ref.generate(s)``, unrounded (its channel lines, restated on its helpers) -- what
    ``nrx_generate_taps`` exports after one float32 rounding, example b U + u"""
    B, U, A, T = s.batch, s.num_tx, s.num_rx_ant, s.num_symbols
    L, NS = s.num_taps, s.num_sinusoids
    slots = s.slot_offset + np.arange(B, dtype=np.int64)
    didx = np.arange(U)[:, None] * L + np.arange(L)[None, :]
    dw = S.draw(s.seed, slots[:, None, None], S.STREAM_DELAY, didx[None])[0]
    tau = np.sort(S.uniform(dw) * s.max_delay_s, axis=-1)
    tau[..., 0] = 0.0
    pdp = np.exp(-tau / (s.max_delay_s / S.PDP_DECAY + 1e-12))
    pdp = pdp / pdp.sum(-1, keepdims=True)
    tidx = (((np.arange(U)[:, None, None, None] * A + np.arange(A)[None, :, None, None]) * L
             + np.arange(L)[None, None, :, None]) * NS + np.arange(NS)[None, None, None, :])
    t0, t1, t2, _ = S.draw(s.seed, slots[:, None, None, None, None], S.STREAM_TAP, tidx[None])
    nre, nim = S.box_muller(t0, t1)
    g0 = (nre + 1j * nim) / np.sqrt(2.0 * NS)
    fd = s.max_doppler_hz * np.cos(2.0 * np.pi * S.uniform(t2))
    tt = np.arange(T) * (S.CP_FACTOR / s.subcarrier_spacing)
    ph = 2.0 * np.pi * (fd[..., None] * tt)
    gt = (g0[..., None] * (np.cos(ph) + 1j * np.sin(ph))).sum(-2)
    return gt * np.sqrt(pdp)[:, :, None, :, None], tau


def as_dataset(gt: np.ndarray, tau: np.ndarray):
    """taps [B, U, A, L, T], delays [B, U, L] -> (a [B U, A, L, T], tau [B U, L], index [B, U]) with example b U + u"""
    B, U = gt.shape[:2]
    return (gt.reshape((B * U,) + gt.shape[2:]), tau.reshape(B * U, -1),
            (np.arange(B)[:, None] * U + np.arange(U)[None, :]).astype(np.int32))


def round_f32(a: np.ndarray, tau: np.ndarray):
    """the dataset as the device holds it: complex64 / float32, widened back exactly"""
    return np.asarray(a).astype(np.complex64).astype(np.complex128), np.asarray(tau).astype(np.float32).astype(np.float64)
