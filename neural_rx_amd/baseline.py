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

from typing import Sequence

from . import _lib
from ._call import fill_grid, fill_mcs, ptr, ref, require, stream_of, torch as _torch
from .generator import NUM_SYMBOLS, GenParams, SlotBatch

SYSTEMS = ("baseline_lsnn_lmmse", "baseline_perf_csi_lmmse")
MAX_TX = 8


class Detector:
    """What the detectors share: ``det(y, h, active, mcs, mcs_bits, no, dmrs_symbols) -> llr
    [1, B, U, F, T, max(mcs_bits)]`` on y [B, F, T, 2A], h [B, U, F, T, 2A] (an estimate or the true
    channel), active [B, U] f32, mcs [B, U] u8 or None (= MCS 0): contiguous tensors on the
    detector's device, in the generator's layouts.  ``err_var`` is added to ``no`` (channel-estimation
    error power seen at a data RE).  Every element of ``out`` is written, so a reused buffer needs no
    clearing.  A subclass names its descriptor (``IO``), adds its own fields and makes the call."""

    IO = None

    def __init__(self, device: int = 0):
        self.device = device
        self._lib = _lib.load()

    def _io(self, y, h, active, mcs, mcs_bits, no, dmrs_symbols, err_var, out):
        """the arguments checked and the part of the descriptor that ``nrx_lmmse_io`` and
        ``nrx_kbest_io`` share filled: ``(io, out)``"""
        torch = _torch()
        B, U, F, T, A2 = h.shape
        dev = torch.device("cuda", self.device)
        require("h", h, dtype=torch.float32, device=dev)
        require("y", y, (B, F, T, A2), torch.float32, dev)
        require("active", active, (B, U), torch.float32, dev)
        if mcs is not None:
            require("mcs", mcs, (B, U), torch.uint8, dev)
        bs = max(mcs_bits)
        if out is None:
            out = torch.empty((1, B, U, F, T, bs), dtype=torch.float32, device=h.device)
        elif tuple(out.shape[:5]) != (1, B, U, F, T) or out.shape[5] < bs or out.dtype != torch.float32 \
                or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 {(1, B, U, F, T)} x >= {bs}")
        io = self.IO()
        fill_grid(io, B, U, F, T, A2 // 2)
        fill_mcs(io, mcs_bits, dmrs_symbols, bits_stride=out.shape[5])
        io.no, io.err_var = float(no), float(err_var)
        io.y, io.h, io.active, io.mcs, io.llr = ptr(y), ptr(h), ptr(active), ptr(mcs), ptr(out)
        return io, out


class LMMSEDetector(Detector):
    """The LMMSE detector with max-log demapping (``nrx_lmmse_detect``); arguments in ``Detector``."""

    IO = _lib.nrx_lmmse_io

    def __call__(self, y, h, active, mcs, mcs_bits: Sequence[int], no: float, dmrs_symbols: Sequence[int],
                 err_var: float = 0.0, out=None, stream=None):
        io, out = self._io(y, h, active, mcs, mcs_bits, no, dmrs_symbols, err_var, out)
        _lib.check(self._lib.nrx_lmmse_detect(ref(io), stream_of(h, stream)))
        return out


class Receiver:
    """What the baseline receivers share: ``rx(sb, no, out=None, stream=None) -> llr [1, B, U, F, T,
    bits_max]`` (``out=None``: the receiver's own buffer, overwritten by the next call of the same batch
    size).  With perfect CSI the detector gets ``sb.h``; otherwise a subclass says which estimate
    (``_estimate``), kept in ``last_h``, and with which ``err_var``."""

    SYSTEMS = ()
    DETECTOR = LMMSEDetector
    KERNEL = "LMMSE kernel is"
    perfect_csi = False

    def __init__(self, system: str, params: GenParams, device: int = 0, **detector_kw):
        if system not in self.SYSTEMS:
            raise ValueError(f"system must be one of {self.SYSTEMS}, got {system!r}")
        if params.num_tx > MAX_TX:
            raise ValueError(f"the {self.KERNEL} built for at most {MAX_TX} users, got {params.num_tx}")
        self.system = system
        self.p = params
        self.detector = self.DETECTOR(device)
        self._detector_kw = detector_kw     # what the subclass passes to every detector call
        self._out = None
        # the channel estimate the last call detected with; None with perfect CSI
        self.last_h = None

    @property
    def _num_active(self) -> int:
        return self.p.num_tx if self.p.num_active is None else self.p.num_active

    @property
    def contaminated(self) -> bool:
        """the LS estimates can be pilot-contaminated: two active ports may share a CDM group"""
        groups = list(self.p.cdm_group[:self.p.num_tx])
        return not self.perfect_csi and self.p.dmrs is None and self._num_active > 1 \
            and max(groups.count(g) for g in set(groups)) > 1

    def __call__(self, sb: SlotBatch, no: float, out=None, stream=None):
        p = self.p
        ev = self.err_var(no)
        if self.perfect_csi:
            h = sb.h
            if h is None:
                raise ValueError(f"{self.system} needs the true channel: SlotGenerator(want_h=True)")
        else:
            h = self.last_h = self._estimate(sb, no, stream)
        if out is None:
            B = h.shape[0]
            if self._out is None or self._out.shape[1] != B:
                torch = _torch()
                self._out = torch.empty((1, B, p.num_tx, p.num_subcarriers, NUM_SYMBOLS, p.bits_max),
                                        dtype=torch.float32, device=h.device)
            out = self._out
        return self.detector(sb.y, h, sb.active, sb.mcs, p.mcs_bits, no, p.dmrs_symbols, err_var=ev, out=out,
                             stream=stream, **self._detector_kw)


class BaselineReceiver(Receiver):
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

    SYSTEMS = SYSTEMS

    def __init__(self, system: str, params: GenParams, device: int = 0):
        super().__init__(system, params, device)
        self.perfect_csi = system == "baseline_perf_csi_lmmse"

    def err_var(self, no: float) -> float:
        if self.perfect_csi:
            return 0.0
        n = 1 if self.p.dmrs is None else self.p.dmrs.block
        return self._num_active * float(no) / (2.0 * n)

    def _estimate(self, sb: SlotBatch, no: float, stream):
        if sb.h_hat is None:
            raise ValueError("the slot batch has no h_hat")
        return sb.h_hat
