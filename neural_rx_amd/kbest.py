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

from typing import Sequence

from . import _lib
from ._call import Workspace, ref, stream_of
from .baseline import Detector, Receiver
from .chest import EstimatorBaselineReceiver
from .generator import GenParams, SlotBatch

SYSTEMS = ("baseline_lmmse_kbest", "baseline_perf_csi_kbest")
MAX_TX = 8
MAX_K = 64


class KBestDetector(Detector):
    """The K-best detector (``nrx_kbest_detect``) on the tensors of ``baseline.Detector``: ``k``
    survivors per level (1..64), LLRs clipped to ``+-llr_clip``.  The detector owns its workspace and
    keeps it from call to call (it grows with the batch); ``workspace=`` (a uint8 tensor on the device,
    at least ``nrx_kbest_workspace_size`` bytes, any content) runs one call in the caller's instead."""

    IO = _lib.nrx_kbest_io

    def __init__(self, device: int = 0):
        super().__init__(device)
        self._ws = Workspace()
        self.last_workspace_bytes = 0      # what nrx_kbest_workspace_size asked for the last call

    def __call__(self, y, h, active, mcs, mcs_bits: Sequence[int], no: float, dmrs_symbols: Sequence[int],
                 err_var: float = 0.0, k: int = MAX_K, llr_clip: float = 20.0, out=None, stream=None,
                 workspace=None):
        io, out = self._io(y, h, active, mcs, mcs_bits, no, dmrs_symbols, err_var, out)
        io.k, io.llr_clip = int(k), float(llr_clip)
        self.last_workspace_bytes = self._ws.size(self._lib.nrx_kbest_workspace_size, ref(io))
        ws = self._ws.get(self.last_workspace_bytes, h.device, workspace)
        _lib.check(self._lib.nrx_kbest_detect(ref(io), ws.data_ptr(), ws.numel(), stream_of(h, stream)))
        return out


class KBestBaselineReceiver(Receiver):
    """``rx(sb, no) -> llr [1, B, U, F, T, bits_max]`` with one of the reference's K-best systems.

    ``baseline_lmmse_kbest``: the estimate of ``chest.ChannelEstimator("lmmse")`` and the scalar
    ``err_var`` of ``chest.EstimatorBaselineReceiver("baseline_lmmse_lmmse")`` (it needs ``R_f`` /
    ``R_t``, here or through ``set_covariance``, and works on LS estimates at the pilots, so it is
    meaningful for at most one active port per CDM group).
    ``baseline_perf_csi_kbest``: ``sb.h`` (the generator must run with ``want_h=True``) and
    ``err_var = 0``.
    ``cfo`` (a ``cfo.CFOCompensator``): the estimator leg runs through it (``chest.ChannelEstimator``)."""

    SYSTEMS = SYSTEMS
    DETECTOR = KBestDetector
    KERNEL = "K-best kernels are"

    def __init__(self, system: str, params: GenParams, device: int = 0, k: int = MAX_K, R_f=None, R_t=None,
                 cfo=None):
        if not 1 <= int(k) <= MAX_K:
            raise ValueError(f"k must be 1..{MAX_K}, got {k}")
        super().__init__(system, params, device, k=int(k))
        self.k = int(k)
        self.perfect_csi = system == "baseline_perf_csi_kbest"
        # the estimator leg is the one of baseline_lmmse_lmmse: same estimate, same err_var
        self._est = None if self.perfect_csi else \
            EstimatorBaselineReceiver("baseline_lmmse_lmmse", params, device, R_f=R_f, R_t=R_t, cfo=cfo)

    def set_covariance(self, R_f, R_t) -> None:
        if self._est is not None:
            self._est.set_covariance(R_f, R_t)

    def err_var(self, no: float) -> float:
        return 0.0 if self._est is None else self._est.err_var(no)

    def _estimate(self, sb: SlotBatch, no: float, stream):
        return self._est.estimator(sb, no, stream=stream)
