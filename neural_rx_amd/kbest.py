"""K-best MIMO detection on the GPU and the reference's two K-best baseline systems.

``baseline_lmmse_kbest`` (2-D LMMSE channel estimation) and ``baseline_perf_csi_kbest`` (the true
channel), both followed by K-best detection with k = 64 (utils/baseline_rx.py:242-254), here the
HIP kernels behind ``nrx_kbest_detect`` (include/nrx.h, csrc/nrx_kbest.hip).  The reference takes
its detector from Sionna and holds no source of it, so the detector is defined by this project
(include/nrx.h has the definition, DESIGN.md section 9 the departures): a real-valued
breadth-first tree over the PAM axes of the users, pinned by the exhaustive max-log ML detector
where the two must coincide.  The LLRs come out in the engine's layout, so
``generator.count_errors`` and ``evaluate.sim_ber_baseline`` read them like every other
receiver's.  Uncoded only: there is no LDPC decoder here.

Everything runs through ``libnrx.so``; torch tensors are only device containers, and a missing
library is an error (``_lib.load``), never a host fallback.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

from . import _lib
from .chest import EstimatorBaselineReceiver
from .generator import NUM_SYMBOLS, GenParams, SlotBatch

SYSTEMS = ("baseline_lmmse_kbest", "baseline_perf_csi_kbest")
MAX_TX = 8
MAX_K = 64


def _torch():
    import torch
    return torch


class KBestDetector:
    """``det(y, h, active, mcs, mcs_bits, no, dmrs_symbols) -> llr [1, B, U, F, T, max(mcs_bits)]``.

    The tensors of ``baseline.LMMSEDetector``: y [B, F, T, 2A], h [B, U, F, T, 2A] (an estimate or
    the true channel), active [B, U] f32, mcs [B, U] u8 or None (= MCS 0), contiguous on the device.
    ``k`` survivors per level (1..64), LLRs clipped to ``+-llr_clip``.  Every element of ``out`` is
    written, so a reused buffer needs no clearing.  The detector owns its workspace and keeps it
    from call to call (it grows with the batch); ``workspace=`` (a uint8 tensor on the device, at
    least ``nrx_kbest_workspace_size`` bytes, any content) runs one call in the caller's instead."""

    def __init__(self, device: int = 0):
        self.device = device
        self._lib = _lib.load()
        self._ws = None
        self.last_workspace_bytes = 0      # what nrx_kbest_workspace_size asked for the last call

    def __call__(self, y, h, active, mcs, mcs_bits: Sequence[int], no: float, dmrs_symbols: Sequence[int],
                 err_var: float = 0.0, k: int = MAX_K, llr_clip: float = 20.0, out=None, stream=None,
                 workspace=None):
        torch = _torch()
        B, U, F, T, A2 = h.shape
        if h.device != torch.device(f"cuda:{self.device}"):
            raise ValueError(f"tensors must be on cuda:{self.device}, h is on {h.device}")
        if tuple(y.shape) != (B, F, T, A2):
            raise ValueError(f"y must be {(B, F, T, A2)}, got {tuple(y.shape)}")
        if tuple(active.shape) != (B, U) or (mcs is not None and tuple(mcs.shape) != (B, U)):
            raise ValueError(f"active / mcs must be {(B, U)}")
        if y.dtype != torch.float32 or h.dtype != torch.float32 or active.dtype != torch.float32:
            raise ValueError("y, h and active must be float32")
        if mcs is not None and mcs.dtype != torch.uint8:
            raise ValueError("mcs must be uint8")
        for t in (y, h, active, mcs):
            if t is not None and not t.is_contiguous():
                raise ValueError("tensors must be contiguous")
        bs = max(mcs_bits)
        if out is None:
            out = torch.empty((1, B, U, F, T, bs), dtype=torch.float32, device=h.device)
        elif tuple(out.shape[:5]) != (1, B, U, F, T) or out.shape[5] < bs or out.dtype != torch.float32 \
                or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 {(1, B, U, F, T)} x >= {bs}")
        io = _lib.nrx_kbest_io()
        io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = B, U, F, T
        io.num_rx_ant, io.bits_stride, io.num_mcs = A2 // 2, out.shape[5], len(mcs_bits)
        for m, b in enumerate(mcs_bits[:8]):
            io.mcs_bits[m] = b
        io.dmrs_symbol_mask = sum(1 << t for t in dmrs_symbols)
        io.k = int(k)
        io.no, io.err_var, io.llr_clip = float(no), float(err_var), float(llr_clip)
        io.y, io.h, io.active, io.llr = y.data_ptr(), h.data_ptr(), active.data_ptr(), out.data_ptr()
        io.mcs = mcs.data_ptr() if mcs is not None else None
        need = ctypes.c_size_t()
        _lib.check(self._lib.nrx_kbest_workspace_size(ctypes.byref(io), ctypes.byref(need)))
        self.last_workspace_bytes = need.value
        if workspace is not None:
            if workspace.device != h.device or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
                raise ValueError(f"workspace must be a contiguous uint8 tensor on {h.device}")
            ws = workspace
        else:
            if self._ws is None or self._ws.numel() < need.value:
                self._ws = torch.empty(need.value, dtype=torch.uint8, device=h.device)
            ws = self._ws
        if stream is None:
            stream = torch.cuda.current_stream(h.device).cuda_stream
        _lib.check(self._lib.nrx_kbest_detect(ctypes.byref(io), ws.data_ptr(), ws.numel(), stream))
        return out


class KBestBaselineReceiver:
    """``rx(sb, no) -> llr [1, B, U, F, T, bits_max]`` with one of the reference's K-best systems.

    ``baseline_lmmse_kbest``: the estimate of ``chest.ChannelEstimator("lmmse")`` and the scalar
    ``err_var`` of ``chest.EstimatorBaselineReceiver("baseline_lmmse_lmmse")`` (it needs ``R_f`` /
    ``R_t``, here or through ``set_covariance``, and works on LS estimates at the pilots, so it is
    meaningful for at most one active port per CDM group).
    ``baseline_perf_csi_kbest``: ``sb.h`` (the generator must run with ``want_h=True``) and
    ``err_var = 0``.
    ``cfo`` (a ``cfo.CFOCompensator``): the estimator leg runs through it (``chest.ChannelEstimator``)."""

    SYSTEMS = SYSTEMS

    def __init__(self, system: str, params: GenParams, device: int = 0, k: int = MAX_K, R_f=None, R_t=None,
                 cfo=None):
        if system not in SYSTEMS:
            raise ValueError(f"system must be one of {SYSTEMS}, got {system!r}")
        if params.num_tx > MAX_TX:
            raise ValueError(f"the K-best kernels are built for at most {MAX_TX} users, got {params.num_tx}")
        if not 1 <= int(k) <= MAX_K:
            raise ValueError(f"k must be 1..{MAX_K}, got {k}")
        self.system = system
        self.p = params
        self.k = int(k)
        self.perfect_csi = system == "baseline_perf_csi_kbest"
        # the estimator leg is the one of baseline_lmmse_lmmse: same estimate, same err_var
        self._est = None if self.perfect_csi else \
            EstimatorBaselineReceiver("baseline_lmmse_lmmse", params, device, R_f=R_f, R_t=R_t, cfo=cfo)
        self.detector = KBestDetector(device)
        self._out = None
        self.last_h = None      # the estimate the last call detected with; None with perfect CSI

    def set_covariance(self, R_f, R_t) -> None:
        if self._est is not None:
            self._est.set_covariance(R_f, R_t)

    @property
    def contaminated(self) -> bool:
        """the LS estimates can be pilot-contaminated: two active ports may share a CDM group"""
        return self._est is not None and self._est.contaminated

    def err_var(self, no: float) -> float:
        return 0.0 if self._est is None else self._est.err_var(no)

    def __call__(self, sb: SlotBatch, no: float, out=None, stream=None):
        p = self.p
        if self.perfect_csi:
            h, ev = sb.h, 0.0
            if h is None:
                raise ValueError("baseline_perf_csi_kbest needs the true channel: SlotGenerator(want_h=True)")
        else:
            ev = self._est.err_var(no)
            h = self.last_h = self._est.estimator(sb, no, stream=stream)
        if out is None:
            B = h.shape[0]
            if self._out is None or self._out.shape[1] != B:
                torch = _torch()
                self._out = torch.empty((1, B, p.num_tx, p.num_subcarriers, NUM_SYMBOLS, p.bits_max),
                                        dtype=torch.float32, device=h.device)
            out = self._out
        return self.detector(sb.y, h, sb.active, sb.mcs, p.mcs_bits, no, p.dmrs_symbols, err_var=ev, k=self.k,
                             out=out, stream=stream)
