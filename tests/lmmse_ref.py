"""numpy statement of the LMMSE + max-log baseline detector (``nrx_lmmse_detect``, include/nrx.h).
A test helper, not a test.

Per resource element (b, f, t), with ``s = no + err_var`` and H [A x U] the channel whose columns
of inactive users (``active <= 0``) are zero:

    G = H^H H + s I,   x^ = G^-1 H^H y,   a_u = (G^-1)_uu,   mu_u = 1 - s a_u,
    x~_u = x^_u / mu_u,   nu_u = s a_u / mu_u          (Sionna ``lmmse_equalizer`` with
                                                        ``whiten_interference``)
    llr_k = (min_{c: b_k = 0} |x~_u - c|^2 - min_{c: b_k = 1} |x~_u - c|^2) / nu_u

over the Gray QAM of ``oracle.synth_ref.qam`` (all 2^m points are searched here; the kernel uses
the per-axis PAM form of the same minimum).  Entries k >= m, inactive users, DMRS symbols and
RE-users with mu_u < 1e-6 are 0.

``dtype=np.float64`` is the reference.  ``dtype=np.float32`` runs the same steps in
float32 / complex64 (LAPACK's single-precision inverse included), rounded at every step: it is used
only to measure the rounding floor of the f32 formulation, reference against reference.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from oracle import synth_ref as S

MU_MIN = 1e-6


def constellation(m: int, dtype=np.float64) -> np.ndarray:
    """points[j] of the 2^m-QAM, bit k of j = bit k of the label"""
    j = np.arange(1 << m)
    bits = ((j[:, None] >> np.arange(m)[None, :]) & 1).astype(np.uint8)
    return S.qam(bits, m).astype(np.complex64 if dtype == np.float32 else np.complex128)


def to_complex(x: np.ndarray, dtype=np.float64) -> np.ndarray:
    """[..., 2A] (Re a0.., Im a0..) -> [..., A] complex of the given real dtype"""
    A = x.shape[-1] // 2
    x = x.astype(dtype)
    return x[..., :A] + 1j * x[..., A:] if dtype == np.float64 else \
        (x[..., :A] + np.complex64(1j) * x[..., A:]).astype(np.complex64)


def lmmse_detect(y: np.ndarray, h: np.ndarray, active: np.ndarray, mcs: Optional[np.ndarray],
                 mcs_bits: Sequence[int], no: float, dmrs_symbols: Sequence[int], err_var: float = 0.0,
                 bits_stride: Optional[int] = None, dtype=np.float64, return_mu: bool = False):
    """y [B, F, T, 2A], h [B, U, F, T, 2A], active [B, U], mcs [B, U] or None ->
    llr [1, B, U, F, T, bits_stride] of ``dtype`` (and mu [B, U, F, T] with ``return_mu``)."""
    B, U, F, T, _ = h.shape
    bs = max(mcs_bits) if bits_stride is None else bits_stride
    real = np.dtype(dtype).type
    s = real(no + err_var)
    one = real(1.0)
    act = np.asarray(active) > 0
    yc = to_complex(y, dtype)                                                  # [B,F,T,A]
    hc = to_complex(h, dtype) * act[:, :, None, None, None].astype(dtype)      # [B,U,F,T,A]
    H = np.moveaxis(hc, 1, -1)                                                 # [B,F,T,A,U]
    Hh = np.conj(np.swapaxes(H, -1, -2))                                       # [B,F,T,U,A]
    G = Hh @ H + s * np.eye(U, dtype=H.dtype)
    Ginv = np.linalg.inv(G)
    assert Ginv.dtype == H.dtype
    xh = (Ginv @ (Hh @ yc[..., None]))[..., 0]                                 # [B,F,T,U]
    a = np.real(np.diagonal(Ginv, axis1=-2, axis2=-1)).astype(dtype)
    sa = s * a
    mu = one - sa
    ok = mu >= real(MU_MIN)
    mu_safe = np.where(ok, mu, one)
    xt = xh / mu_safe.astype(H.dtype)
    nu = sa / mu_safe
    xt = np.moveaxis(xt, -1, 1)                                                # [B,U,F,T]
    nu = np.moveaxis(nu, -1, 1)
    ok = np.moveaxis(ok, -1, 1)
    mu = np.moveaxis(mu, -1, 1)
    llr = np.zeros((1, B, U, F, T, bs), dtype)
    data = np.ones(T, bool)
    data[list(dmrs_symbols)] = False
    mcs = np.zeros((B, U), np.int64) if mcs is None else np.asarray(mcs).astype(np.int64)
    for mi, m in enumerate(mcs_bits):
        sel = (mcs == mi) & act                                                # [B,U]
        if not sel.any():
            continue
        pts = constellation(m, dtype)
        d = xt[..., None] - pts                                                # [B,U,F,T,2^m]
        d = (d.real * d.real + d.imag * d.imag).astype(dtype)
        lab = np.arange(1 << m)
        for k in range(m):
            one_k = ((lab >> k) & 1).astype(bool)
            v = (d[..., ~one_k].min(-1) - d[..., one_k].min(-1)) / nu
            keep = sel[:, :, None, None] & ok & data[None, None, None, :]
            llr[0, ..., k] = np.where(keep, v, llr[0, ..., k])
    return (llr, mu) if return_mu else llr


# ---- the cases of tests/test_gpu_lmmse.py (and their CPU counts in tests/test_lmmse_ref.py) ------
# name: (U, A, F, mcs_bits, drawn MCS, Eb/N0 dB, B, num_active, dmrs symbols,
#        {csi: (bit errors, bits)} of the f64 reference on oracle.synth_ref.generate, err_var = 0)
CASES = {
    "C1": (2, 4, 12, (4,), False, 6.0, 3, None, (2, 11), {"ls": (342, 3456), "perfect": (144, 3456)}),
    "C2": (8, 4, 12, (6,), False, 10.0, 2, None, (2, 11), {"perfect": (5088, 13824)}),
    "C3": (4, 16, 12, (2, 4, 6), True, 12.0, 4, 2, (2, 11), {"ls": (2, 4032), "perfect": (0, 4032)}),
    "C4": (1, 2, 13, (2,), False, 4.0, 1, None, (2,), {"ls": (39, 338), "perfect": (20, 338)}),
    "C5": (2, 4, 12, (4,), False, 8.0, 5, None, (2, 11), {"ls": (432, 5760), "perfect": (143, 5760)}),
    "C6": (3, 4, 12, (4,), False, 8.0, 2, None, (2, 11), {"perfect": (119, 3456)}),
    # U = 5, 6, 7 with dwordx4 / dwordx2 loads (A = 8) and with scalar loads (A % 4 != 0)
    "C7": (5, 8, 12, (4,), False, 8.0, 2, None, (2, 11), {"perfect": (27, 5760)}),
    "C8": (6, 8, 12, (6,), False, 12.0, 2, None, (2, 11), {"perfect": (437, 10368)}),
    "C9": (7, 8, 12, (2,), False, 2.0, 2, None, (2, 11), {"perfect": (71, 4032)}),
    "C10": (5, 6, 12, (4,), False, 8.0, 2, None, (2, 11), {"perfect": (169, 5760)}),
    "C11": (6, 10, 12, (4,), False, 8.0, 2, None, (2, 11), {"perfect": (19, 6912)}),
    "C12": (7, 10, 12, (6,), False, 12.0, 2, None, (2, 11), {"perfect": (184, 12096)}),
    # U = 1 with dwordx4 loads (C4 is its scalar twin)
    "C13": (1, 4, 12, (2,), False, 4.0, 2, None, (2, 11), {"perfect": (4, 576)}),
}
SEED = 7


def case_spec(name: str) -> S.GenSpec:
    """The oracle generator spec of a case: seed 7, cdm_group[u] = u % 2, no from Eb/N0."""
    U, A, F, mcs_bits, drawn, ebno, B, na, dmrs, _ = CASES[name]
    return S.GenSpec(batch=B, num_tx=U, num_subcarriers=F, num_rx_ant=A, dmrs_symbols=dmrs,
                     cdm_group=tuple(u % 2 for u in range(U)), mcs_bits=mcs_bits,
                     mcs_of_user=[-1 if drawn else 0] * U, num_active=na,
                     no=S.ebno_to_no(ebno, len(dmrs)), seed=SEED)
