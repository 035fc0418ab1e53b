"""numpy statements of the channel-estimation baselines (``nrx_cov_accumulate``, ``nrx_chest_lmmse``,
``nrx_chest_lin``: include/nrx.h, neural_rx_amd/chest.py).  A test helper, not a test.

``dtype=np.float64`` is the reference; ``dtype=np.float32`` runs the same steps in float32 /
complex64 and only measures the rounding floor of an f32 formulation, reference against reference.

The 2-D LMMSE filter is stated here in its brute-force form, the Kronecker solve
``(R_t[:, D] (x) R_f[:, P]) (R_t[D, D] (x) R_f[P, P] + sigma^2 I)^-1`` -- deliberately not the eigen
form of ``chest.lmmse_design``, so that the two are independent formulations.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

T = 14

# name: (U, A, F, DMRS symbols, B, num_active) -- the cases of tests/test_gpu_chest.py
CASES = {
    "K1": (2, 4, 24, (2, 11), 3, None),       # the bench model's geometry
    "K2": (1, 2, 13, (2,), 1, None),          # odd F, one DMRS symbol, group sizes 7 / 6, partial tiles
    "K3": (4, 16, 36, (2, 7, 11), 2, 2),      # nd = 3, 2A = 32, inactive users
    "K4": (2, 4, 132, (2, 11), 2, None),      # several M tiles, K = 264 not a tile multiple
    "K5": (2, 1, 12, (2, 11), 2, None),       # 2A = 2
    "K6": (2, 4, 24, (2, 3, 10, 11), 2, None),    # nd = 4 (two double-symbol DMRS), vector stores
    "K7": (2, 3, 24, (2, 3, 10, 11), 2, None),    # nd = 4, scalar stores
    "K8": (2, 4, 24, (2,), 2, None),              # nd = 1 with vector stores (K2 is its scalar twin)
}
SEED = 7
EBNO_DB = 5.0


def to_complex(x: np.ndarray, dtype=np.float64) -> np.ndarray:
    """[..., 2A] (Re a0.., Im a0..) -> [..., A] complex of the given real dtype"""
    A = x.shape[-1] // 2
    c = np.complex128 if dtype == np.float64 else np.complex64
    x = x.astype(dtype)
    return (x[..., :A] + c(1j) * x[..., A:]).astype(c)


def to_channels(z: np.ndarray) -> np.ndarray:
    return np.concatenate([z.real, z.imag], axis=-1)


def lag_sums(h: np.ndarray):
    """h [B, U, F, T, 2A] f32 -> (sf [F], st [14]) complex128:
    sf[d] = sum_{b,u,a,t} sum_{f < F - d} h[f + d] conj(h[f]), st[d] likewise along t."""
    hc = to_complex(h)
    F = hc.shape[2]
    sf = np.array([np.sum(hc[:, :, d:] * np.conj(hc[:, :, :F - d])) for d in range(F)])
    st = np.array([np.sum(hc[:, :, :, d:] * np.conj(hc[:, :, :, :T - d])) for d in range(T)])
    return sf, st


def lag_counts(B: int, U: int, F: int, A: int):
    """number of products in every lag: (frequency [F], time [14])"""
    return B * U * A * T * (F - np.arange(F)), B * U * A * F * (T - np.arange(T))


def toeplitz(lags: np.ndarray) -> np.ndarray:
    n = len(lags)
    R = np.zeros((n, n), np.complex128)
    for i in range(n):
        for j in range(n):
            R[i, j] = lags[i - j] if i >= j else np.conj(lags[j - i])
    return R


def model_covariance(F: int, max_delay_s=300e-9, scs=30e3, max_doppler_hz=400.0, n=64):
    """A positive semi-definite Toeplitz (R_f, R_t) of the generator's kind of channel: an
    exponential power-delay profile over [0, max_delay) and uniform Doppler angles."""
    tau = (np.arange(n) + 0.5) / n * max_delay_s
    w = np.exp(-tau / (max_delay_s / 3.0))
    w /= w.sum()
    r_f = np.array([np.sum(w * np.exp(-2j * np.pi * d * scs * tau)) for d in range(F)])
    fd = max_doppler_hz * np.cos(2 * np.pi * (np.arange(n) + 0.5) / n)
    tsym = (1.0 + 9.0 / 128.0) / scs
    r_t = np.array([np.mean(np.exp(2j * np.pi * fd * d * tsym)) for d in range(T)])
    return toeplitz(r_f), toeplitz(r_t)


def pilots(F: int, group: int) -> np.ndarray:
    return np.array([f for f in range(F) if f % 2 == group], np.int64)


def lmmse_filter_brute(R_f: np.ndarray, R_t: np.ndarray, dmrs: Sequence[int], group: int, no: float):
    """(W [F, T, nd, |P|], err [F, T]): h^[f, t] = sum_{d, p} W[f, t, d, p] h_ls[P_p, D_d], the
    Kronecker solve with sigma^2 = no / 2 and R_t scaled to a unit diagonal; err = prior - diag(W C^H)."""
    F = R_f.shape[0]
    D, P = list(dmrs), pilots(F, group)
    R_t = R_t / R_t[0, 0].real
    C = np.kron(R_t[:, D], R_f[:, P])                               # rows (t, f), columns (d, p)
    Cpp = np.kron(R_t[np.ix_(D, D)], R_f[np.ix_(P, P)])
    W = C @ np.linalg.inv(Cpp + (no / 2.0) * np.eye(len(D) * len(P)))
    err = R_f[0, 0].real - np.real(np.sum(W * np.conj(C), axis=1))
    W = W.reshape(T, F, len(D), len(P)).transpose(1, 0, 2, 3)
    return W, err.reshape(T, F).T


def lmmse_brute(h_hat, active, R_f, R_t, dmrs, cdm_group, no):
    """the brute-force estimate [B, U, F, T, 2A] in float64"""
    B, U, F = h_hat.shape[:3]
    x = to_complex(h_hat)
    out = np.zeros_like(x)
    for u in range(U):
        W, _ = lmmse_filter_brute(R_f, R_t, dmrs, cdm_group[u], no)
        hls = x[:, u][:, pilots(F, cdm_group[u])][:, :, list(dmrs)]          # [B, P, nd, A]
        out[:, u] = np.einsum("ftdp,bpda->bfta", W, hls)
    out *= (np.asarray(active) > 0)[:, :, None, None, None]
    return to_channels(out)


def lmmse_apply(h_hat, active, filt, tcoef, vconj, dmrs, cdm_group, dtype=np.float64):
    """The estimate from given tables (chest.LMMSEDesign: filt [2, nd, F, Pmax, 2], tcoef
    [nd, 14, 2], vconj [nd, nd, 2]) in ``dtype`` arithmetic: z_k = sum_d vconj[k][d] h_ls[P, D_d],
    h^[f, t] = sum_k tcoef[k][t] (filt[group][k] z_k)[f]."""
    B, U, F = h_hat.shape[:3]
    c = np.complex128 if dtype == np.float64 else np.complex64
    cx = lambda a: (a[..., 0].astype(dtype) + c(1j) * a[..., 1].astype(dtype)).astype(c)  # noqa: E731
    W, a, v = cx(filt), cx(tcoef), cx(vconj)
    x = to_complex(h_hat, dtype)
    out = np.zeros(x.shape, c)
    for u in range(U):
        P = pilots(F, cdm_group[u])
        if not len(P):
            continue
        hls = x[:, u][:, P][:, :, list(dmrs)]                                # [B, P, nd, A]
        for k in range(len(dmrs)):
            z = np.einsum("d,bpda->bpa", v[k], hls).astype(c)
            y = np.matmul(W[cdm_group[u], k][:, :len(P)], z).astype(c)       # [B, F, A]
            out[:, u] += (a[k][None, None, :, None] * y[:, :, None, :]).astype(c)
    out *= (np.asarray(active) > 0)[:, :, None, None, None].astype(dtype)
    return to_channels(out).astype(dtype)


def lin_interp(h_hat, active, dmrs, cdm_group, dtype=np.float64):
    """Linear interpolation of the LS estimates at the own pilots (include/nrx.h nrx_chest_lin):
    along f between the bracketing pilots (the two nearest ones beyond the band edges), then along
    t between the bracketing DMRS symbols; a single pilot or symbol is repeated."""
    B, U, F = h_hat.shape[:3]
    real = np.dtype(dtype).type
    x = to_complex(h_hat, dtype)
    out = np.zeros_like(x)
    D = list(dmrs)
    t0, t1, wt = np.zeros(T, int), np.zeros(T, int), np.zeros(T, dtype)
    for t in range(T):
        if len(D) == 1:
            t0[t] = t1[t] = D[0]
            continue
        k = max([i for i in range(len(D) - 1) if D[i] <= t], default=0)
        t0[t], t1[t] = D[k], D[k + 1]
        wt[t] = real(t - D[k]) / real(D[k + 1] - D[k])
    for u in range(U):
        P = pilots(F, cdm_group[u])
        if not len(P):
            continue
        p0, p1, wf = np.zeros(F, int), np.zeros(F, int), np.zeros(F, dtype)
        for f in range(F):
            if len(P) == 1:
                p0[f] = p1[f] = P[0]
                continue
            j = max([i for i in range(len(P) - 1) if P[i] <= f], default=0)
            p0[f], p1[f] = P[j], P[j + 1]
            wf[f] = real(0.5) * real(f - P[j])
        one = real(1.0)
        uf, vf = (one - wf)[None, :, None, None], wf[None, :, None, None]
        ut, vt = (one - wt)[None, None, :, None], wt[None, None, :, None]
        xu = x[:, u]
        g = lambda pp, tt: xu[:, pp][:, :, tt]                               # noqa: E731  [B, F, T, A]
        out[:, u] = ut * (uf * g(p0, t0) + vf * g(p1, t0)) + vt * (uf * g(p0, t1) + vf * g(p1, t1))
    out *= (np.asarray(active) > 0)[:, :, None, None, None].astype(dtype)
    return to_channels(out).astype(dtype)
