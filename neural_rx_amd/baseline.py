"""Classical baseline receivers on the GPU: LS or perfect CSI + LMMSE detection + max-log demapping.

The counterpart of the reference's ``BaselineReceiver`` (utils/baseline_rx.py:44-303) for the
two systems whose pieces exist here -- ``baseline_lsnn_lmmse`` (LS estimates at the pilots +
nearest-neighbour interpolation, which the slot generator already writes as ``h_hat``) and
``baseline_perf_csi_lmmse`` (the true channel) -- both followed by Sionna's
``LinearDetector("lmmse", "bit", "maxlog")`` (baseline_rx.py:262-272), here the HIP kernel behind
``nrx_lmmse_detect`` (include/nrx.h, csrc/nrx_lmmse.hip).  The LLRs come out in the engine's
layout, so ``generator.count_errors`` and ``evaluate.sim_ber_baseline`` read them like the
neural receiver's.  Uncoded only: there is no LDPC decoder here.

Everything runs through ``libnrx.so``; torch tensors are only device containers, and a missing
library is an error (``_lib.load``), never a host fallback.

Limit of the LS baseline.  The slot generator applies no orthogonal cover code, so ports that
share a CDM group send their pilots on the same REs and each one's ``h_hat`` is the sum of their
channels (pilot contamination).  The neural receiver is trained to resolve that; a linear detector
fed with such an estimate is not (8 users / 4 antennas at 10 dB: BER 0.46).  ``baseline_lsnn_lmmse``
is therefore meaningful for at most one active port per CDM group (U <= 2 with groups 0 / 1);
``baseline_perf_csi_lmmse`` is meaningful for any U.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

from . import _lib
from .generator import NUM_SYMBOLS, GenParams, SlotBatch

SYSTEMS = ("baseline_lsnn_lmmse", "baseline_perf_csi_lmmse")
MAX_TX = 8


def _torch():
    import torch
    return torch


class LMMSEDetector:
    """``det(y, h, active, mcs, mcs_bits, no, dmrs_symbols) -> llr [1, B, U, F, T, max(mcs_bits)]``.

    y [B, F, T, 2A], h [B, U, F, T, 2A] (an estimate or the true channel), active [B, U] f32,
    mcs [B, U] u8 or None (= MCS 0): contiguous device tensors in the generator's layouts.
    ``err_var`` is added to ``no`` (channel-estimation error power seen at a data RE).  Every
    element of ``out`` is written, so a reused buffer needs no clearing."""

    def __init__(self, device: int = 0):
        self.device = device
        self._lib = _lib.load()

    def __call__(self, y, h, active, mcs, mcs_bits: Sequence[int], no: float, dmrs_symbols: Sequence[int],
                 err_var: float = 0.0, out=None, stream=None):
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
        io = _lib.nrx_lmmse_io()
        io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = B, U, F, T
        io.num_rx_ant, io.bits_stride, io.num_mcs = A2 // 2, out.shape[5], len(mcs_bits)
        for m, b in enumerate(mcs_bits[:8]):
            io.mcs_bits[m] = b
        io.dmrs_symbol_mask = sum(1 << t for t in dmrs_symbols)
        io.no, io.err_var = float(no), float(err_var)
        io.y, io.h, io.active, io.llr = y.data_ptr(), h.data_ptr(), active.data_ptr(), out.data_ptr()
        io.mcs = mcs.data_ptr() if mcs is not None else None
        if stream is None:
            stream = torch.cuda.current_stream(h.device).cuda_stream
        _lib.check(self._lib.nrx_lmmse_detect(ctypes.byref(io), stream))
        return out


class BaselineReceiver:
    """``rx(sb, no) -> llr``: a ``SlotBatch`` and its noise variance to LLRs
    ``[1, B, U, F, T, bits_max]`` with one of the reference's baseline systems.

    ``baseline_lsnn_lmmse``: ``sb.h_hat`` and ``err_var = num_active * no / 2`` -- the generator's
    pilots have energy 2, so the LS error of each active user has variance ``no / 2`` per antenna,
    and at a data RE those errors (times unit-energy symbols) add to the noise.  Meaningful for
    at most one active port per CDM group (module docstring) -- unless the ports carry cover codes
    (``GenParams.dmrs``): ``sb.h_hat`` is then the despread estimate over ``n = dmrs.block`` pilots
    (1, 2 or 4), ``err_var = num_active * no / (2 n)``, and ports of one group are separated.
    ``baseline_perf_csi_lmmse``: ``sb.h`` (the generator must run with ``want_h=True``) and
    ``err_var = 0``."""

    def __init__(self, system: str, params: GenParams, device: int = 0):
        if system not in SYSTEMS:
            raise ValueError(f"system must be one of {SYSTEMS}, got {system!r}")
        if params.num_tx > MAX_TX:
            raise ValueError(f"the LMMSE kernel is built for at most {MAX_TX} users, got {params.num_tx}")
        self.system = system
        self.p = params
        self.perfect_csi = system == "baseline_perf_csi_lmmse"
        self.detector = LMMSEDetector(device)
        self._out = None
        # the channel estimate the last call detected with (sb.h_hat); None with perfect CSI
        self.last_h = None

    @property
    def contaminated(self) -> bool:
        """the LS estimate can be pilot-contaminated: two active ports may share a CDM group"""
        p = self.p
        na = p.num_tx if p.num_active is None else p.num_active
        groups = list(p.cdm_group[:p.num_tx])
        return not self.perfect_csi and p.dmrs is None and na > 1 and max(groups.count(g) for g in set(groups)) > 1

    def err_var(self, no: float) -> float:
        if self.perfect_csi:
            return 0.0
        na = self.p.num_tx if self.p.num_active is None else self.p.num_active
        n = 1 if self.p.dmrs is None else self.p.dmrs.block
        return na * float(no) / (2.0 * n)

    def __call__(self, sb: SlotBatch, no: float, out=None, stream=None):
        p = self.p
        h = sb.h if self.perfect_csi else sb.h_hat
        if h is None:
            raise ValueError("baseline_perf_csi_lmmse needs the true channel: SlotGenerator(want_h=True)"
                             if self.perfect_csi else "the slot batch has no h_hat")
        self.last_h = None if self.perfect_csi else h
        if out is None:
            B = h.shape[0]
            if self._out is None or self._out.shape[1] != B:
                torch = _torch()
                self._out = torch.empty((1, B, p.num_tx, p.num_subcarriers, NUM_SYMBOLS, p.bits_max),
                                        dtype=torch.float32, device=h.device)
            out = self._out
        return self.detector(sb.y, h, sb.active, sb.mcs, p.mcs_bits, no, p.dmrs_symbols,
                             err_var=self.err_var(no), out=out, stream=stream)
