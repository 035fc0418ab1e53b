"""numpy statements of the 3-D LMMSE channel estimator (``nrx_chest_lmmse3``: include/nrx.h,
``chest.lmmse3_design``).  A test helper, not a test; the conventions are those of
tests/chest_ref.py (``dtype=np.float64`` is the reference, ``dtype=np.float32`` measures the rounding
floor of an f32 formulation, reference against reference).

The filter is stated twice: ``lmmse3_brute`` is the Kronecker solve
``C (C_obs + sigma^2 I)^-1`` with ``C = R_s (x) R_t[:, D] (x) R_f[:, P]`` -- deliberately not the
spectral form -- and ``lmmse3_apply`` applies given tables as the header defines them.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from tests.chest_ref import T, pilots, to_channels, to_complex

# name: (U, A, F, DMRS symbols, B, num_active, R_s kind) -- the cases of tests/test_gpu_chest3.py
CASES = {
    "K1": (2, 4, 24, (2, 11), 3, None, "corr"),         # the bench model's geometry, alpha = 0.9
    "K2": (1, 2, 13, (2,), 1, None, "corr"),            # odd F, one DMRS symbol, 7 / 6 pilots, partial tiles
    "K3": (4, 16, 36, (2, 7, 11), 2, 2, "corr"),        # nd = 3, N a full tile, inactive users
    "K4": (2, 3, 132, (2, 11), 2, None, "random"),      # several M tiles, complex non-symmetric V_s, K = 66
    "K5": (2, 1, 12, (2, 11), 2, None, "corr"),         # A = 1
    "K6": (2, 4, 24, (2, 3, 10, 11), 2, None, "corr"),  # nd = 4 (two double-symbol DMRS)
    "K7": (2, 4, 24, (2,), 2, None, "corr"),            # nd = 1 with vector stores (K2 is its scalar twin)
}


def normalise(R_t: np.ndarray, R_s: np.ndarray):
    """R_t to a unit diagonal, R_s to trace A: the scaling of chest.lmmse3_design"""
    return R_t / R_t[0, 0].real, R_s * (R_s.shape[0] / np.trace(R_s).real)


def lmmse3_filter_brute(R_f, R_t, R_s, dmrs: Sequence[int], group: int, no: float):
    """(W [A F T, A nd |P|], C, C_obs): rows (a, t, f), columns (a', d, p); ``W = C (C_obs +
    sigma^2 I)^-1`` with sigma^2 = no / 2."""
    F = R_f.shape[0]
    D, P = list(dmrs), pilots(F, group)
    R_t, R_s = normalise(np.asarray(R_t, np.complex128), np.asarray(R_s, np.complex128))
    C = np.kron(R_s, np.kron(R_t[:, D], R_f[:, P]))
    Cobs = np.kron(R_s, np.kron(R_t[np.ix_(D, D)], R_f[np.ix_(P, P)]))
    W = C @ np.linalg.inv(Cobs + (no / 2.0) * np.eye(Cobs.shape[0]))
    return W, C, Cobs


def err_brute(R_f, R_t, R_s, dmrs, group, no):
    """diag(C_hh - W C^H) as [A, F, T]: the error variance of the Kronecker filter"""
    F, A = R_f.shape[0], R_s.shape[0]
    W, C, _ = lmmse3_filter_brute(R_f, R_t, R_s, dmrs, group, no)
    _, Rs = normalise(np.asarray(R_t, np.complex128), np.asarray(R_s, np.complex128))
    prior = np.repeat(np.real(np.diag(Rs)), T * F) * R_f[0, 0].real
    err = prior - np.real(np.sum(W * np.conj(C), axis=1))
    return err.reshape(A, T, F).transpose(0, 2, 1)


def lmmse3_brute(h_hat, active, R_f, R_t, R_s, dmrs, cdm_group, no):
    """the brute-force estimate [B, U, F, T, 2A] in float64"""
    B, U, F = h_hat.shape[:3]
    x = to_complex(h_hat)                                                   # [B, U, F, T, A]
    A = x.shape[-1]
    out = np.zeros_like(x)
    for u in range(U):
        P = pilots(F, cdm_group[u])
        if not len(P):
            continue
        W, _, _ = lmmse3_filter_brute(R_f, R_t, R_s, dmrs, cdm_group[u], no)
        hls = x[:, u][:, P][:, :, list(dmrs)]                               # [B, P, nd, A]
        obs = hls.transpose(0, 3, 2, 1).reshape(B, -1)                      # (a', d, p)
        est = (obs @ W.T).reshape(B, A, T, F)
        out[:, u] = est.transpose(0, 3, 2, 1)
    out *= (np.asarray(active) > 0)[:, :, None, None, None]
    return to_channels(out)


def lmmse3_apply(h_hat, active, tables, dmrs, cdm_group, no, dtype=np.float64):
    """The estimate from given tables (chest.LMMSE3Design or any object with its fields) in ``dtype``
    arithmetic, as include/nrx.h states it:
        w[j,k,q] = sum_a conj(vs[a][j]) sum_d vconj[k][d] sum_p qh[g][q][p] h_ls[a, P_p, D_d]
        c[j,k,q] = mu_j / (mu_j lam_k nu_q + sigma^2) w[j,k,q]
        h^[a,f,t] = sum_j vs[a][j] sum_k tcoef[k][t] sum_q gf[g][f][q] c[j,k,q]"""
    B, U, F = h_hat.shape[:3]
    c = np.complex128 if dtype == np.float64 else np.complex64
    cx = lambda a: (a[..., 0].astype(dtype) + c(1j) * a[..., 1].astype(dtype)).astype(c)  # noqa: E731
    qh, gf, tc, vc, vs = (cx(getattr(tables, k)) for k in ("qh", "gf", "tcoef", "vconj", "vs"))
    nu, lam, mu = (getattr(tables, k).astype(dtype) for k in ("nu", "lam", "mu"))
    sigma2 = dtype(np.float32(no / 2.0)) if dtype == np.float32 else dtype(no / 2.0)
    x = to_complex(h_hat, dtype)
    out = np.zeros(x.shape, c)
    for u in range(U):
        g = cdm_group[u]
        P = pilots(F, g)
        n = len(P)
        if not n:
            continue
        hls = x[:, u][:, P][:, :, list(dmrs)]                               # [B, P, nd, A]
        z = np.einsum("aj,kd,bpda->bjkp", vs.conj(), vc, hls).astype(c)
        w = np.einsum("qp,bjkp->bjkq", qh[g][:n, :n], z).astype(c)
        gain = (mu[:, None, None] / (mu[:, None, None] * lam[None, :, None] * nu[g][None, None, :n] + sigma2)).astype(dtype)
        cc = (w * gain[None]).astype(c)
        y = np.einsum("fq,bjkq->bjkf", gf[g][:, :n], cc).astype(c)
        out[:, u] = np.einsum("aj,kt,bjkf->bfta", vs, tc, y).astype(c)
    out *= (np.asarray(active) > 0)[:, :, None, None, None].astype(dtype)
    return to_channels(out).astype(dtype)
