"""numpy statement of the K-best MIMO detector (``nrx_kbest_detect``, include/nrx.h) and the
exhaustive max-log ML detector it is pinned by.  A test helper, not a test.

Per data resource element (b, f, t), with ``s = no + err_var``:

1. streams: the n users with ``active > 0`` in port order; user u sends m_u bits of the Gray QAM
   of ``oracle.synth_ref.qam`` (even bits on the real axis, odd bits on the imaginary axis), each
   axis a PAM of L_u = 2^(m_u / 2) levels (level index j: bit q of j is the axis' q-th bit);
2. real model: y_r = [Re y; Im y], user u has the columns [Re h; Im h] (Re x_u) and
   [-Im h; Re h] (Im x_u);
3. order: users by ||h_u||^2 ascending (ties: lower u first), streams
   [Re u(1), Im u(1), Re u(2), ...]; detection runs from the last stream to the first;
4. G = H^T H = R^T R (R upper triangular, positive diagonal, no regularisation),
   y~ = R^-T H^T y_r; a pivot d_i <= 1e-6 G_ii makes every LLR of the RE 0;
5. search: one empty path of metric 0; at level i = 2n-1 .. 0 every survivor expands into the L
   children of stream i with metric + (y~_i - sum_{j>i} R_ij x_j - R_ii a)^2 / s, and the K
   smallest survive (stable order at ties);
6. llr[u][k] = clip(min_{b_k = 0} metric - min_{b_k = 1} metric, +-llr_clip) over the final list,
   a side without a path counting as +inf.

Entries k >= m_u, inactive users and DMRS symbols are 0.  ``dtype=np.float64`` is the reference;
``dtype=np.float32`` runs every step (the Cholesky included) in float32 and is used only to
measure the rounding floor of the f32 formulation, reference against reference.
"""
from __future__ import annotations

import itertools
from typing import Optional, Sequence

import numpy as np

from oracle import synth_ref as S

PIVOT_MIN = 1e-6
SCALE = {2: 1.0 / np.sqrt(2.0), 4: 1.0 / np.sqrt(10.0), 6: 1.0 / np.sqrt(42.0)}


def pam(m: int, dtype=np.float64) -> np.ndarray:
    """levels[j] of one axis of the 2^m-QAM, bit q of j = the axis' q-th bit (8 entries, the
    ones past 2^(m/2) are 0)"""
    nb = m // 2
    j = np.arange(8)
    s = [1.0 - 2.0 * ((j >> q) & 1) for q in range(3)]
    lev = s[0] if nb == 1 else (s[0] * (2.0 - s[1]) if nb == 2 else s[0] * (4.0 - s[1] * (2.0 - s[2])))
    lev = np.where(j < (1 << nb), lev * SCALE[m], 0.0)
    return lev.astype(dtype)


def _real_model(y, h, dtype):
    """y [N, 2A], h [N, n, 2A] (Re a0.., Im a0..) -> y_r [N, 2A], H [N, 2A, 2n] in stream order
    [Re u0, Im u0, Re u1, ...]"""
    A = y.shape[-1] // 2
    hr, hi = h[..., :A], h[..., A:]
    col_re = np.concatenate([hr, hi], -1)                       # [N, n, 2A]
    col_im = np.concatenate([-hi, hr], -1)
    H = np.stack([col_re, col_im], 2).reshape(h.shape[0], -1, 2 * A)   # [N, 2n, 2A]
    return y.astype(dtype), np.swapaxes(H, 1, 2).astype(dtype)


def _cholesky_upper(G, z):
    """G [N, d, d], z [N, d] -> R (G = R^T R), y~ = R^-T z, min pivot ratio d_i / G_ii, degenerate
    mask; every step in G's dtype.  Degenerate REs get a unit pivot so the rest stays finite."""
    N, d, _ = G.shape
    real = G.dtype.type
    R = np.zeros_like(G)
    yt = np.zeros_like(z)
    bad = np.zeros(N, bool)
    ratio = np.full(N, np.inf)
    for i in range(d):
        num = G[:, i, i:].copy()
        rhs = z[:, i].copy()
        for k in range(i):
            num -= R[:, k, i, None] * R[:, k, i:]
            rhs -= R[:, k, i] * yt[:, k]
        piv = num[:, 0]
        gii = G[:, i, i]
        deg = ~(piv > real(PIVOT_MIN) * gii)
        bad |= deg
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.minimum(ratio, np.where(gii > 0, piv / np.where(gii > 0, gii, real(1)), -np.inf))
        rii = np.sqrt(np.where(deg, real(1), piv))
        R[:, i, i:] = num / rii[:, None]
        R[:, i, i] = rii
        yt[:, i] = rhs / rii
    return R, yt, ratio, bad


def kbest_detect(y: np.ndarray, h: np.ndarray, active: np.ndarray, mcs: Optional[np.ndarray],
                 mcs_bits: Sequence[int], no: float, dmrs_symbols: Sequence[int], err_var: float = 0.0,
                 k: int = 64, llr_clip: float = 20.0, bits_stride: Optional[int] = None, dtype=np.float64,
                 return_pivot: bool = False):
    """y [B, F, T, 2A], h [B, U, F, T, 2A], active [B, U], mcs [B, U] or None ->
    llr [1, B, U, F, T, bits_stride] of ``dtype`` (and the minimum pivot ratio d_i / G_ii over the
    data REs with ``return_pivot``)."""
    B, U, F, T, A2 = h.shape
    bs = max(mcs_bits) if bits_stride is None else bits_stride
    real = np.dtype(dtype).type
    s = real(no + err_var)
    clip = real(llr_clip)
    act = np.asarray(active) > 0
    mcs = np.zeros((B, U), np.int64) if mcs is None else np.asarray(mcs).astype(np.int64)
    data = np.array([t for t in range(T) if t not in set(dmrs_symbols)])
    llr = np.zeros((1, B, U, F, T, bs), dtype)
    min_ratio = np.inf
    for b in range(B):
        users = np.nonzero(act[b])[0]
        n = len(users)
        if n == 0 or len(data) == 0:
            continue
        N = F * len(data)
        yb = y[b][:, data].reshape(N, A2).astype(dtype)
        hb = np.moveaxis(h[b][users][:, :, data], 0, 2).reshape(N, n, A2).astype(dtype)   # [N, n, 2A]
        # order: ascending column energy, ties by port (stable sort of the port-ordered list)
        order = np.argsort((hb * hb).sum(-1), axis=1, kind="stable")               # [N, n] -> position in users
        hp = np.take_along_axis(hb, order[:, :, None], 1)
        m_pos = np.array(mcs_bits)[mcs[b, users]][order]                           # [N, n] bits of the p-th user
        yr, H = _real_model(yb, hp, dtype)
        G = np.swapaxes(H, 1, 2) @ H
        z = (np.swapaxes(H, 1, 2) @ yr[:, :, None])[:, :, 0]
        assert G.dtype == np.dtype(dtype)
        R, yt, ratio, bad = _cholesky_upper(G, z)
        min_ratio = min(min_ratio, float(ratio.min()))
        d = 2 * n
        tables = {m: pam(m, dtype) for m in set(mcs_bits)}
        amp = np.zeros((N, n, 8), dtype)                                           # levels of the p-th user
        for m, tb in tables.items():
            amp[m_pos == m] = tb
        nlev = 1 << (m_pos // 2)                                                   # [N, n]
        # survivors: metric [N, C], level indices [N, C, d], amplitudes [N, C, d]
        lam = np.zeros((N, 1), dtype)
        idx = np.zeros((N, 1, d), np.int64)
        xs = np.zeros((N, 1, d), dtype)
        inf = real(np.inf)
        for i in range(d - 1, -1, -1):
            p = i // 2
            r = yt[:, i, None] - (R[:, None, i, i + 1:] * xs[:, :, i + 1:]).sum(-1, dtype=dtype) \
                if i + 1 < d else np.broadcast_to(yt[:, i, None], lam.shape)
            e = r[:, :, None] - R[:, i, i, None, None] * amp[:, None, p, :]         # [N, C, 8]
            cand = lam[:, :, None] + e * e / s
            cand = np.where(np.arange(8)[None, None, :] < nlev[:, p, None, None], cand, inf)
            C = lam.shape[1]
            keep = min(k, C * int(nlev[:, p].max()))
            sel = np.argsort(cand.reshape(N, C * 8), axis=1, kind="stable")[:, :keep]
            par, ch = sel // 8, sel % 8
            lam = np.take_along_axis(cand.reshape(N, C * 8), sel, 1)
            idx = np.take_along_axis(idx, par[:, :, None], 1)
            xs = np.take_along_axis(xs, par[:, :, None], 1)
            idx[:, :, i] = ch
            xs[:, :, i] = np.take_along_axis(amp[:, p, :], ch, 1)
        out = np.zeros((N, n, bs), dtype)
        for p in range(n):
            for kb in range(min(6, bs)):
                lev = idx[:, :, 2 * p + (kb & 1)]
                one = ((lev >> (kb >> 1)) & 1).astype(bool)
                m0 = np.where(~one, lam, inf).min(1)
                m1 = np.where(one, lam, inf).min(1)
                with np.errstate(invalid="ignore"):
                    v = np.clip(m0 - m1, -clip, clip)
                out[:, p, kb] = np.where((kb < m_pos[:, p]) & ~bad, v, real(0))
        # back to port order
        res = np.zeros((N, n, bs), dtype)
        np.put_along_axis(res, order[:, :, None], out, 1)
        res = np.moveaxis(res.reshape(F, len(data), n, bs), 2, 0)                  # [n, F, Td, bs]
        for q, u in enumerate(users):
            llr[0, b, u][:, data] = res[q]
    return (llr, min_ratio) if return_pivot else llr


def ml_detect(y: np.ndarray, h: np.ndarray, active: np.ndarray, mcs: Optional[np.ndarray],
              mcs_bits: Sequence[int], no: float, dmrs_symbols: Sequence[int], err_var: float = 0.0,
              llr_clip: float = 20.0, bits_stride: Optional[int] = None) -> np.ndarray:
    """Exhaustive max-log ML in float64, straight from y and H:
    llr[u][k] = clip(min_{x: b_k = 0} |y - H x|^2 / s - min_{x: b_k = 1} |y - H x|^2 / s)."""
    B, U, F, T, A2 = h.shape
    A = A2 // 2
    bs = max(mcs_bits) if bits_stride is None else bits_stride
    s = float(no + err_var)
    act = np.asarray(active) > 0
    mcs = np.zeros((B, U), np.int64) if mcs is None else np.asarray(mcs).astype(np.int64)
    data = np.array([t for t in range(T) if t not in set(dmrs_symbols)])
    llr = np.zeros((1, B, U, F, T, bs))
    for b in range(B):
        users = np.nonzero(act[b])[0]
        if len(users) == 0 or len(data) == 0:
            continue
        ms = [mcs_bits[mcs[b, u]] for u in users]
        yc = y[b][:, data].astype(np.float64)
        yc = yc[..., :A] + 1j * yc[..., A:]                                        # [F, Td, A]
        hc = h[b][users][:, :, data].astype(np.float64)
        hc = hc[..., :A] + 1j * hc[..., A:]                                        # [n, F, Td, A]
        labels = np.array(list(itertools.product(*[range(1 << m) for m in ms])))   # [P, n]
        x = np.zeros(labels.shape, np.complex128)
        for q, m in enumerate(ms):
            lab = labels[:, q]
            bits = ((lab[:, None] >> np.arange(m)[None, :]) & 1).astype(np.uint8)
            x[:, q] = S.qam(bits, m)
        hx = np.einsum("nfta,pn->ftpa", hc, x)
        met = (np.abs(yc[:, :, None, :] - hx) ** 2).sum(-1) / s                    # [F, Td, P]
        for q, u in enumerate(users):
            for kb in range(ms[q]):
                one = ((labels[:, q] >> kb) & 1).astype(bool)
                v = met[..., ~one].min(-1) - met[..., one].min(-1)
                llr[0, b, u][:, data, kb] = np.clip(v, -llr_clip, llr_clip)
    return llr


# ---- the cases of tests/test_gpu_kbest.py (and their CPU counts in tests/test_kbest_ref.py) ------
# name: (U, A, F, mcs_bits, drawn MCS, Eb/N0 dB, B, num_active, dmrs symbols, exhaustive at k = 64,
#        (K-best bit errors, LMMSE bit errors, bits) of the f64 references on
#        oracle.synth_ref.generate with perfect CSI, err_var = 0, k = 64, llr_clip = 20)
CASES = {
    "K1": (1, 2, 12, (6,), False, 8.0, 2, None, (2, 11), True, (299, 299, 1728)),
    "K2": (3, 4, 12, (2,), False, 4.0, 2, None, (2, 11), True, (9, 22, 1728)),
    "K3": (4, 4, 12, (4,), False, 10.0, 3, None, (2, 11), False, (156, 457, 6912)),
    "K4": (2, 4, 12, (6,), False, 14.0, 3, None, (2, 11), False, (66, 90, 5184)),
    "K5": (8, 8, 12, (2,), False, -2.0, 2, None, (2, 11), False, (107, 335, 4608)),
    "K6": (4, 16, 12, (2, 4, 6), True, 0.0, 4, 2, (2, 11), False, (103, 116, 4032)),
    # U = 5, 6, 7 (10, 12, 14 levels) with vector Gram loads, and U = 5 with an odd antenna count
    "K7": (5, 8, 12, (2,), False, 0.0, 2, None, (2, 11), False, (5, 29, 2880)),
    "K8": (6, 8, 12, (2,), False, 0.0, 2, None, (2, 11), False, (5, 70, 3456)),
    "K9": (7, 8, 12, (2,), False, 0.0, 2, None, (2, 11), False, (7, 123, 4032)),
    "K10": (5, 5, 12, (4,), False, 10.0, 2, None, (2, 11), False, (30, 328, 5760)),
    # 456 * 12 * 12 = 65 664 data REs, 128 more than the search grid holds: some waves take a second RE
    "K11": (2, 4, 12, (2,), False, 2.0, 456, None, (2, 11), True, (4376, 6181, 262656)),
}
# K6 runs at 0 dB: at 12 dB (two active users on sixteen antennas) 99.8 % of its LLRs sit on the clip
# and test no arithmetic.
PRUNED = [n for n in CASES if not CASES[n][9]]
SEED = 7


def case_spec(name: str) -> S.GenSpec:
    """The oracle generator spec of a case: seed 7, cdm_group[u] = u % 2, no from Eb/N0."""
    U, A, F, mcs_bits, drawn, ebno, B, na, dmrs, _, _ = CASES[name]
    return S.GenSpec(batch=B, num_tx=U, num_subcarriers=F, num_rx_ant=A, dmrs_symbols=dmrs,
                     cdm_group=tuple(u % 2 for u in range(U)), mcs_bits=mcs_bits,
                     mcs_of_user=[-1 if drawn else 0] * U, num_active=na,
                     no=S.ebno_to_no(ebno, len(dmrs)), seed=SEED)
