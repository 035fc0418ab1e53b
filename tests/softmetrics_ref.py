"""numpy statement of the soft-output sums (``nrx_llr_stats`` / ``nrx_chest_nmse``, include/nrx.h).
A test helper, not a test.  float64 throughout, on the same f32 inputs as the kernels.

Contributing set: (slot b, user u) with ``active > 0``, symbols not in ``dmrs_symbols``, every
subcarrier, bit positions ``k < mcs_bits[mcs[b, u]]`` (MCS 0 without ``mcs``); head ``mcs[b, u]`` when
the LLR tensor has more than one head.  For a contributing finite LLR ``L`` with sent bit ``c`` and
scale ``s``: ``z = (2c - 1) s L`` and ``loss = logaddexp(0, -z) / ln 2`` bits (= ``(max(-z, 0) +
log1p(exp(-|z|))) / ln 2``).  A NaN / inf LLR is counted in ``nonfinite`` only.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

K = 8


def llr_stats(llr: np.ndarray, bits: np.ndarray, active: np.ndarray, mcs: Optional[np.ndarray],
              mcs_bits: Sequence[int], dmrs_symbols: Sequence[int], scales: Sequence[float]):
    """llr [H, B, U, F, T, bs] f32, bits [B, U, F, T, bs] u8, active [B, U], mcs [B, U] or None ->
    loss [U, M, 8, S] f64 (bits), cnt [U, M, 8] i64, nonfinite [U, M, 8] i64."""
    H, B, U, F, T, _ = llr.shape
    M, S = len(mcs_bits), len(scales)
    loss = np.zeros((U, M, K, S), np.float64)
    cnt = np.zeros((U, M, K), np.int64)
    nonfinite = np.zeros((U, M, K), np.int64)
    data = np.ones(T, bool)
    data[list(dmrs_symbols)] = False
    sc = np.asarray(scales, np.float64)
    for b in range(B):
        for u in range(U):
            if not active[b, u] > 0:
                continue
            m = int(mcs[b, u]) if mcs is not None else 0
            nb = mcs_bits[m]
            L = llr[m if H > 1 else 0, b, u][:, data, :nb].astype(np.float64)       # [F, Td, nb]
            c = bits[b, u][:, data, :nb].astype(np.float64)
            fin = np.isfinite(L)
            z = (2.0 * c - 1.0) * np.where(fin, L, 0.0)
            lo = np.logaddexp(0.0, -z[..., None] * sc) / np.log(2.0)                # [F, Td, nb, S]
            loss[u, m, :nb] += (lo * fin[..., None]).sum((0, 1))
            cnt[u, m, :nb] += fin.sum((0, 1))
            nonfinite[u, m, :nb] += (~fin).sum((0, 1))
    return loss, cnt, nonfinite


def chest_nmse(h_est: np.ndarray, h_true: np.ndarray, active: np.ndarray, symbol_mask: int = 0):
    """h_est, h_true [B, U, F, T, 2A] f32 -> err [U] f64, ref [U] f64, items [U] i64 over the active
    (b, u) and the symbols whose bit is set in ``symbol_mask`` (0: all)."""
    B, U, F, T, _ = h_true.shape
    sel = np.array([(symbol_mask >> t) & 1 if symbol_mask else 1 for t in range(T)], bool)
    act = np.asarray(active) > 0
    d = h_est[:, :, :, sel].astype(np.float64) - h_true[:, :, :, sel].astype(np.float64)
    e = (d * d).sum((2, 3, 4)) * act
    r = (h_true[:, :, :, sel].astype(np.float64) ** 2).sum((2, 3, 4)) * act
    return e.sum(0), r.sum(0), act.sum(0).astype(np.int64)


def bmi_cells(loss: np.ndarray, cnt: np.ndarray) -> np.ndarray:
    """bmi [M, 8, S] = 1 - sum_u loss / sum_u cnt, NaN where nothing was counted"""
    lo, cn = loss.sum(0), cnt.sum(0).astype(np.float64)[..., None]
    return 1.0 - np.divide(lo, cn, out=np.full(lo.shape, np.nan), where=cn > 0)
