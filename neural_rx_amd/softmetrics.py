"""Soft-output metrics of an evaluation: bitwise and generalised mutual information of the LLRs,
and the NMSE of a channel estimate.

The error counters (``generator.count_errors``) look at the sign of an LLR only.  What a decoder
sees is its magnitude.  The quantity that summarises it without a code (the coded BLER itself is
``ldpc.py``) is the *bitwise mutual information* (BMI; Sionna's
``BitwiseMutualInformation``): 1 minus the binary cross-entropy the reference trains on
(neural_rx.py:687), in bits -- the rate a BICM decoder achieves with exactly these LLRs.  The Eb/N0
at which it crosses the code rate predicts the waterfall (``ebno_at_rate``).  The *generalised*
mutual information (GMI) is the best BMI under one LLR scale factor: it separates "wrong
information" from "right information, wrong confidence".  The NMSE places a channel estimate (the
engine's ``h_ref``, or a baseline estimator's) against the true channel of the generator.

The sums run on the GPU through ``libnrx.so`` (``nrx_llr_stats`` / ``nrx_chest_nmse``,
include/nrx.h, where the contributing set and the loss are defined); a missing library is an error.
The accumulators are torch tensors; ``SoftAccumulator(device=None)`` keeps them on the host, for a
caller that fills them itself and only wants ``reduce`` / ``result``.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._call import Workspace, fill_grid, fill_mcs, ptr, ref, stream_of, torch as _torch

DEFAULT_SCALES = (0.25, 0.354, 0.5, 0.707, 1.0, 1.414, 2.0, 2.828, 4.0)
MAX_SCALES = 16
MAX_BITS = 8
STRIP_SUBCARRIERS = _lib.SOFT_STRIP


def ebno_at_rate(curve, rate: float) -> Optional[float]:
    """Eb/N0 at which a mutual-information curve reaches ``rate``: ``curve`` is a sequence of
    ``(ebno_db, value)`` points in sweep order; the result is the linear interpolation of the first
    crossing from below ``rate`` to at or above it (a first point exactly at ``rate`` counts), or
    None if there is none.  The caller supplies the code rate: the project carries no rate table."""
    pts = [(float(e), float(v)) for e, v in curve]
    if pts and pts[0][1] == rate:
        return pts[0][0]
    for (e0, v0), (e1, v1) in zip(pts, pts[1:]):
        if v0 < rate <= v1:
            return e0 + (rate - v0) / (v1 - v0) * (e1 - e0)
    return None


def _ratio(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.full(np.broadcast(num, den).shape, np.nan), where=den > 0)


def _nan_none(x):
    """nested lists with NaN as None (JSON has no NaN)"""
    if isinstance(x, dict):
        return {k: _nan_none(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_nan_none(v) for v in x]
    if isinstance(x, float) and x != x:
        return None
    return x


@dataclasses.dataclass
class SoftResult:
    """Host-side figures of one set of accumulators.  Cells without a contributing LLR are NaN
    (``as_dict``: None).  ``m`` indexes the MCS, ``k`` the bit position, ``s`` the scale, ``u`` the user."""
    scales: List[float]
    mcs_bits: List[int]
    bmi: List[float]                  # [m] count-weighted mean over k < bits[m], at the scale nearest 1.0
    bmi_bits: List                    # [m][k][s] = 1 - sum_u loss / sum_u cnt (may be negative)
    gmi: List[float]                  # [m] max over s of the same mean over k
    gmi_scale: List[float]            # [m] the scale of that maximum
    cnt: List                         # [m][k] contributing finite LLRs
    nonfinite: int                    # NaN / +-inf LLRs in the contributing set
    nonfinite_bits: List              # [m][k]
    nmse: Optional[float]             # sum_u err / sum_u ref; None if no channel estimate was scored
    bmi_user: List                    # [u][m]
    gmi_user: List                    # [u][m]
    gmi_scale_user: List              # [u][m]
    nmse_user: Optional[List]         # [u]
    channel_items: int                # (slot, user) grids behind the NMSE

    def as_dict(self):
        return _nan_none(dataclasses.asdict(self))


def derive(loss, cnt, nonfinite, mcs_bits: Sequence[int], scales: Sequence[float], err=None, ref=None,
           items=None) -> SoftResult:
    """``SoftResult`` of accumulator arrays: loss [U, M, 8, S] f64, cnt / nonfinite [U, M, 8] i64, and
    (optionally) err / ref [U] f64 with items [U] i64 (include/nrx.h)."""
    loss, cnt, nonfinite = np.asarray(loss, np.float64), np.asarray(cnt, np.int64), np.asarray(nonfinite, np.int64)
    U, M, K, S = loss.shape
    scales = [float(s) for s in scales]
    s1 = int(np.argmin(np.abs(np.asarray(scales) - 1.0)))
    used = np.arange(K)[None, :] < np.asarray(mcs_bits)[:, None]                 # [M, K]

    def means(lo, cn):
        """[..., M, K, S] / [..., M, K] -> bmi [..., M], gmi [..., M], gmi scale [..., M]"""
        per_s = 1.0 - _ratio((lo * used[..., None]).sum(-2), (cn * used).sum(-1)[..., None])   # [..., M, S]
        ok = ~np.isnan(per_s[..., 0])
        best = np.argmax(np.where(np.isnan(per_s), -np.inf, per_s), axis=-1)
        gmi = np.take_along_axis(per_s, best[..., None], -1)[..., 0]
        return per_s[..., s1], gmi, np.where(ok, np.asarray(scales)[best], np.nan)

    bmi, gmi, gsc = means(loss.sum(0), cnt.sum(0))
    bmi_u, gmi_u, gsc_u = means(loss, cnt)
    bmi_bits = 1.0 - _ratio(loss.sum(0), cnt.sum(0)[..., None])
    nmse = nmse_user = None
    n_items = 0
    if err is not None and items is not None and int(np.sum(items)) > 0:
        err, ref = np.asarray(err, np.float64), np.asarray(ref, np.float64)
        nmse = float(err.sum() / ref.sum()) if ref.sum() > 0 else float("nan")
        nmse_user = _ratio(err, ref).tolist()
        n_items = int(np.sum(items))
    return SoftResult(scales=scales, mcs_bits=[int(b) for b in mcs_bits], bmi=bmi.tolist(),
                      bmi_bits=bmi_bits.tolist(), gmi=gmi.tolist(), gmi_scale=gsc.tolist(),
                      cnt=cnt.sum(0).tolist(), nonfinite=int(nonfinite.sum()),
                      nonfinite_bits=nonfinite.sum(0).tolist(), nmse=nmse, bmi_user=bmi_u.tolist(),
                      gmi_user=gmi_u.tolist(), gmi_scale_user=gsc_u.tolist(), nmse_user=nmse_user,
                      channel_items=n_items)


class SoftAccumulator:
    """Device accumulators of ``nrx_llr_stats`` / ``nrx_chest_nmse`` for ``num_tx`` users and the MCS
    list ``mcs_bits``, with their workspace.  ``add_llr`` / ``add_channel`` are asynchronous on the
    stream; ``reduce`` sums over the ranks of a process group; ``result`` copies to the host.

    The int64 accumulators (cnt, nonfinite, items) are views of one tensor ``i64`` and the float64
    ones (loss, err, ref) of one tensor ``f64``, so that a reduction is one collective each."""

    def __init__(self, num_tx: int, mcs_bits: Sequence[int], scales: Sequence[float] = DEFAULT_SCALES,
                 device: Optional[int] = 0):
        torch = _torch()
        scales = [float(s) for s in scales]
        if not 1 <= len(scales) <= MAX_SCALES or not all(np.isfinite(s) and s > 0 for s in scales):
            raise ValueError(f"scales must be 1..{MAX_SCALES} finite positive numbers, got {scales}")
        if not 1 <= len(mcs_bits) <= 8 or not all(1 <= int(b) <= MAX_BITS for b in mcs_bits):
            raise ValueError(f"mcs_bits must be 1..8 widths of 1..{MAX_BITS} bits, got {list(mcs_bits)}")
        self.num_tx, self.mcs_bits, self.scales = int(num_tx), [int(b) for b in mcs_bits], scales
        self.device = device
        dev = "cpu" if device is None else f"cuda:{device}"
        U, M, S = self.num_tx, len(self.mcs_bits), len(scales)
        n = U * M * MAX_BITS
        self.i64 = torch.zeros(2 * n + U, dtype=torch.int64, device=dev)
        self.f64 = torch.zeros(n * S + 2 * U, dtype=torch.float64, device=dev)
        self.cnt = self.i64[:n].view(U, M, MAX_BITS)
        self.nonfinite = self.i64[n:2 * n].view(U, M, MAX_BITS)
        self.items = self.i64[2 * n:]
        self.loss = self.f64[:n * S].view(U, M, MAX_BITS, S)
        self.err = self.f64[n * S:n * S + U]
        self.ref = self.f64[n * S + U:]
        self._ws = Workspace()
        self.last_workspace_bytes = 0      # what the *_workspace_size call asked for the last add_*
        self._total = None         # (i64, f64) of the last reduce, dropped by the next add
        self._lib = _lib.load() if device is not None else None

    def _run(self, size_fn, fn, io, key, given, stream):
        """``fn(io)`` in the workspace, grown to what ``size_fn(io)`` asks for (asked once per shape
        ``key``) -- or in the caller's ``workspace=`` (a uint8 tensor on the device, any content)"""
        self.last_workspace_bytes = self._ws.size(size_fn, ref(io), key=key)
        ws = self._ws.get(self.last_workspace_bytes, self.i64.device, given)
        _lib.check(fn(ref(io), ws.data_ptr(), ws.numel(), stream))
        self._total = None

    def _on_device(self, **tensors):
        if self._lib is None:
            raise RuntimeError("a host SoftAccumulator (device=None) has no kernels: fill its tensors directly")
        for name, t in tensors.items():
            if t is not None and (t.device != self.i64.device or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous tensor on {self.i64.device}")

    def add_llr(self, llr, bits, active, mcs, dmrs_symbols: Sequence[int], stream=None, workspace=None):
        """llr [H, B, U, F, T, bits_stride] f32 (head = MCS if H > 1), bits [B, U, F, T, bits_stride] u8,
        active [B, U] f32, mcs [B, U] u8 or None (= MCS 0)."""
        torch = _torch()
        self._on_device(llr=llr, bits=bits, active=active, mcs=mcs)
        H, B, U, F, T, bs = llr.shape
        if U != self.num_tx:
            raise ValueError(f"llr has {U} users, the accumulator {self.num_tx}")
        if tuple(bits.shape) != (B, U, F, T, bs) or bits.dtype != torch.uint8:
            raise ValueError(f"bits must be uint8 {(B, U, F, T, bs)}, got {bits.dtype} {tuple(bits.shape)}")
        if tuple(active.shape) != (B, U) or active.dtype != torch.float32 or llr.dtype != torch.float32:
            raise ValueError(f"llr and active must be float32, active {(B, U)}")
        if mcs is not None and (tuple(mcs.shape) != (B, U) or mcs.dtype != torch.uint8):
            raise ValueError(f"mcs must be uint8 {(B, U)}")
        io = _lib.nrx_llr_stats_io()
        fill_grid(io, B, U, F, T)
        fill_mcs(io, self.mcs_bits, dmrs_symbols, bits_stride=bs, num_heads=H)
        io.num_scales = len(self.scales)
        for s, v in enumerate(self.scales):
            io.scales[s] = v
        io.llr, io.bits, io.active, io.mcs = ptr(llr), ptr(bits), ptr(active), ptr(mcs)
        io.loss, io.cnt, io.nonfinite = ptr(self.loss), ptr(self.cnt), ptr(self.nonfinite)
        self._run(self._lib.nrx_llr_stats_workspace_size, self._lib.nrx_llr_stats, io, ("llr", B, F), workspace,
                  stream_of(llr, stream))

    def add_channel(self, h_est, h_true, active, symbol_mask: int = 0, stream=None, workspace=None):
        """h_est, h_true [B, U, F, T, 2A] f32, active [B, U] f32; ``symbol_mask`` bit t selects symbol t
        (0: all 14)."""
        torch = _torch()
        self._on_device(h_est=h_est, h_true=h_true, active=active)
        B, U, F, T, A2 = h_true.shape
        if U != self.num_tx:
            raise ValueError(f"h_true has {U} users, the accumulator {self.num_tx}")
        if tuple(h_est.shape) != (B, U, F, T, A2) or h_est.dtype != torch.float32 or h_true.dtype != torch.float32:
            raise ValueError(f"h_est and h_true must be float32 {(B, U, F, T, A2)}")
        if tuple(active.shape) != (B, U) or active.dtype != torch.float32:
            raise ValueError(f"active must be float32 {(B, U)}")
        io = _lib.nrx_nmse_io()
        fill_grid(io, B, U, F, T, A2 // 2)
        io.symbol_mask = int(symbol_mask)
        io.h_est, io.h_true, io.active = ptr(h_est), ptr(h_true), ptr(active)
        io.err, io.ref, io.items = ptr(self.err), ptr(self.ref), ptr(self.items)
        self._run(self._lib.nrx_nmse_workspace_size, self._lib.nrx_chest_nmse, io, ("nmse", B, F), workspace,
                  stream_of(h_true, stream))

    def reduce(self, dist=None):
        """Sum the accumulators over the ranks of ``dist`` (``torch.distributed``, or None: this rank
        alone): one all-reduce of the int64 block and one of the float64 block, on host tensors unless
        the backend is nccl.  The local accumulators keep this rank's sums; ``result`` / ``arrays``
        report the totals of the last reduce until the next ``add_*``."""
        i64, f64 = self.i64.clone(), self.f64.clone()
        if dist is not None:
            if dist.get_backend() != "nccl":
                i64, f64 = i64.cpu(), f64.cpu()
            dist.all_reduce(i64)
            dist.all_reduce(f64)
        self._total = (i64.cpu(), f64.cpu())
        return self

    def arrays(self) -> dict:
        """The totals (of the last ``reduce``, else this rank's) as numpy arrays."""
        i64, f64 = self._total if self._total is not None else (self.i64.cpu(), self.f64.cpu())
        i64, f64 = i64.numpy(), f64.numpy()
        U, M, S = self.num_tx, len(self.mcs_bits), len(self.scales)
        n = U * M * MAX_BITS
        return dict(cnt=i64[:n].reshape(U, M, MAX_BITS), nonfinite=i64[n:2 * n].reshape(U, M, MAX_BITS),
                    items=i64[2 * n:], loss=f64[:n * S].reshape(U, M, MAX_BITS, S), err=f64[n * S:n * S + U],
                    ref=f64[n * S + U:])

    def result(self) -> SoftResult:
        a = self.arrays()
        return derive(a["loss"], a["cnt"], a["nonfinite"], self.mcs_bits, self.scales, a["err"], a["ref"],
                      a["items"])
