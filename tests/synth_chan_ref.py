"""numpy float64 statement of ``nrx_generate_slots_ex`` (include/nrx.h): the slot generator of
``oracle/synth_ref.py`` with per-port delay / Doppler spreads and receive-antenna mixing.  A test
helper, not a test.

It restates ``oracle.synth_ref.generate`` on that module's helpers with exactly two changes:

* port ``u`` draws its delays and its PDP constant from ``max_delay_s[u]`` and its Doppler
  frequencies from ``max_doppler_hz[u]`` (the Philox streams and counters are unchanged);
* after the taps ``g[b, u, a, l, t]`` are complete (PDP scaling included) they are mixed over the
  antennas, ``g'[a] = sum_a' M[a][a'] g[a']`` in complex float64 with ``a'`` ascending.

Everything downstream (``h``, ``y``, ``h_hat``) follows from the mixed taps.  With the spec's own
scalars for every port and ``rx_mix=None`` the result equals ``oracle.synth_ref.generate`` bit for
bit (tests/test_synth_chan_ref.py).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from oracle import synth_ref as S


def hermitian_sqrt(R: np.ndarray) -> np.ndarray:
    """``V diag(sqrt(mu)) V^H`` of a Hermitian PSD matrix (negative rounding residues count as 0)"""
    mu, V = np.linalg.eigh(np.asarray(R, np.complex128))
    return (V * np.sqrt(np.maximum(mu, 0.0))) @ V.conj().T


def random_psd(A: int, seed: int) -> np.ndarray:
    """a random complex Hermitian positive definite [A, A] matrix of trace A"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((A, 2 * A)) + 1j * rng.standard_normal((A, 2 * A))
    R = X @ X.conj().T
    return R * (A / np.trace(R).real)


def generate(s: S.GenSpec, user_profiles: Optional[Sequence] = None, rx_mix: Optional[np.ndarray] = None) -> S.GenOut:
    """``user_profiles``: per port ``(max_delay_s, max_doppler_hz)``, None = the spec's scalars;
    ``rx_mix``: complex [A, A] ``M``, None = no mixing."""
    B, U, F, A, T = s.batch, s.num_tx, s.num_subcarriers, s.num_rx_ant, s.num_symbols
    L, NS, M = s.num_taps, s.num_sinusoids, len(s.mcs_bits)
    if user_profiles is None:
        user_profiles = [(s.max_delay_s, s.max_doppler_hz)] * U
    assert len(user_profiles) == U
    max_delay = np.array([p[0] for p in user_profiles], np.float64)         # [U]
    max_doppler = np.array([p[1] for p in user_profiles], np.float64)
    slots = s.slot_offset + np.arange(B, dtype=np.int64)
    dm = np.zeros(T, bool)
    dm[list(s.dmrs_symbols)] = True

    na = U if s.num_active is None else s.num_active
    w = np.stack(S.draw(s.seed, slots[:, None], S.STREAM_ACTIVE, np.arange(4)[None, :]), -1).reshape(B, 16)
    active = np.zeros((B, U), np.float32)
    for b in range(B):
        arr = [1 if i < na else 0 for i in range(U)]
        for i in range(U - 1, 0, -1):
            j = int(w[b, i] % np.uint64(i + 1))
            arr[i], arr[j] = arr[j], arr[i]
        active[b] = arr

    mou = np.array(list(s.mcs_of_user) if s.mcs_of_user is not None else [0] * U)
    wm = S.draw(s.seed, slots[:, None], S.STREAM_MCS, np.arange(U)[None, :])[0]
    mcs = np.where(mou[None, :] >= 0, mou[None, :], (wm % np.uint64(M)).astype(np.int64)).astype(np.uint8)
    nbits = np.array(s.mcs_bits)[mcs]

    idx = (np.arange(U)[:, None, None] * F + np.arange(F)[None, :, None]) * T + np.arange(T)[None, None, :]
    w0, w1, _, _ = S.draw(s.seed, slots[:, None, None, None], S.STREAM_RE, idx[None])
    kk = np.arange(s.bits_max, dtype=np.uint64)
    bits = ((w0[..., None] >> kk) & np.uint64(1)).astype(np.uint8)
    keep = (np.arange(s.bits_max)[None, None, None, None, :] < nbits[:, :, None, None, None])
    keep = keep & ~dm[None, None, None, :, None]
    bits = (bits * keep).astype(np.uint8)
    x = np.zeros((B, U, F, T), np.complex128)
    for m_i, m in enumerate(s.mcs_bits):
        x = np.where((mcs == m_i)[:, :, None, None], S.qam(bits, m), x)
    x[:, :, :, dm] = 0
    pb = np.stack([w1 & np.uint64(1), (w1 >> np.uint64(1)) & np.uint64(1)], -1)
    pil = S.qam(pb.astype(np.uint8), 2) * np.sqrt(2.0)
    own = (np.arange(F)[None, :] % 2) == np.array(s.cdm_group)[:U, None]
    pmask = own[None, :, :, None] & dm[None, None, None, :]
    x = np.where(pmask, pil, x)
    x = x * active[:, :, None, None]

    # channel: delays / PDP per (slot, user), from the port's own max_delay_s
    didx = np.arange(U)[:, None] * L + np.arange(L)[None, :]
    dw = S.draw(s.seed, slots[:, None, None], S.STREAM_DELAY, didx[None])[0]
    tau = np.sort(S.uniform(dw) * max_delay[None, :, None], axis=-1)        # [B,U,L]
    tau[..., 0] = 0.0
    pdp = np.exp(-tau / (max_delay[None, :, None] / S.PDP_DECAY + 1e-12))
    pdp = pdp / pdp.sum(-1, keepdims=True)
    tidx = (((np.arange(U)[:, None, None, None] * A + np.arange(A)[None, :, None, None]) * L
             + np.arange(L)[None, None, :, None]) * NS + np.arange(NS)[None, None, None, :])
    t0, t1, t2, _ = S.draw(s.seed, slots[:, None, None, None, None], S.STREAM_TAP, tidx[None])
    nre, nim = S.box_muller(t0, t1)
    g0 = (nre + 1j * nim) / np.sqrt(2.0 * NS)
    fd = max_doppler[None, :, None, None, None] * np.cos(2.0 * np.pi * S.uniform(t2))   # the port's own Doppler
    tsym = S.CP_FACTOR / s.subcarrier_spacing
    tt = np.arange(T) * tsym
    ph = 2.0 * np.pi * (fd[..., None] * tt)
    gt = (g0[..., None] * (np.cos(ph) + 1j * np.sin(ph))).sum(-2)          # [B,U,A,L,T]
    gt = gt * np.sqrt(pdp)[:, :, None, :, None]
    if rx_mix is not None:                                                  # g'[a] = sum_a' M[a][a'] g[a'], a' ascending
        Mx = np.asarray(rx_mix, np.complex128)
        assert Mx.shape == (A, A)
        mixed = np.zeros_like(gt)
        for a2 in range(A):
            mixed += Mx[None, None, :, a2, None, None] * gt[:, :, a2:a2 + 1]
        gt = mixed
    fa = 2.0 * np.pi * ((np.arange(F)[None, None, None, :] * s.subcarrier_spacing) * tau[..., None])
    e = np.cos(fa) - 1j * np.sin(fa)
    h = np.einsum("bualt,bulf->buaft", gt, e)

    nidx = (np.arange(A)[:, None, None] * F + np.arange(F)[None, :, None]) * T + np.arange(T)[None, None, :]
    n0, n1, _, _ = S.draw(s.seed, slots[:, None, None, None], S.STREAM_NOISE, nidx[None])
    zr, zi = S.box_muller(n0, n1)
    sd = np.sqrt(s.no / 2.0)
    y_c = np.einsum("buaft,buft->baft", h, x) + sd * (zr + 1j * zi)

    def to_ch(z):
        z = np.moveaxis(z, -3, -1)
        return np.concatenate([z.real, z.imag], axis=-1).astype(np.float32)

    y = to_ch(y_c)
    yr = y[..., :A].astype(np.float64) + 1j * y[..., A:].astype(np.float64)
    h_hat = np.zeros((B, U, F, T, A), np.complex128)
    for u in range(U):
        fp, tp = S.nearest_pilot(F, s.dmrs_symbols, s.cdm_group[u], T)
        xp = x[:, u, fp, tp]
        yp = yr[:, fp, tp, :]
        safe = np.where(xp != 0, xp, 1.0)
        h_hat[:, u] = np.where((xp != 0)[..., None], yp / safe[..., None], 0)
    h_hat_ch = np.concatenate([h_hat.real, h_hat.imag], axis=-1).astype(np.float32)
    return S.GenOut(y=y, h_hat=h_hat_ch, h=to_ch(h), active=active, mcs=mcs, bits=bits, x=x, y_c=y_c)


def spatial_sums(h: np.ndarray) -> np.ndarray:
    """h [B, U, F, T, 2A] f32 -> complex128 [A, A]: sum_{b,u,f,t} h[a] conj(h[a'])
    (include/nrx.h nrx_cov_space_accumulate)"""
    A = h.shape[-1] // 2
    hc = (h[..., :A].astype(np.float64) + 1j * h[..., A:].astype(np.float64)).reshape(-1, A)
    return np.einsum("ra,rc->ac", hc, hc.conj())
