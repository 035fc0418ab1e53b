"""Channel-estimation baselines on the GPU: covariance estimation, 2-D LMMSE and linear interpolation.

The counterpart of the estimators of the reference's ``BaselineReceiver`` (utils/baseline_rx.py:
100-229) for ``baseline_lmmse_lmmse`` and ``baseline_lslin_lmmse``, and of its
``scripts/compute_cov_mat.py`` (which ``scripts/evaluate.py:159`` runs before every baseline
evaluation).  The device work is in ``libnrx.so`` (``nrx_cov_accumulate``, ``nrx_chest_lmmse``,
``nrx_chest_lin``: include/nrx.h, csrc/nrx_chest.hip); torch tensors are only device containers and
a missing library is an error, never a host fallback.  The filter design is host numpy float64, run
once per noise level: it is not hot.

Three stated departures from the reference (Sionna):

* **Toeplitz covariance.**  ``CovarianceEstimator`` estimates lags, not full matrices: the
  generator's channel is stationary in frequency and time by construction (oracle/synth_ref.py:
  206-226), so ``R_f`` and ``R_t`` are Hermitian Toeplitz and the lags estimate the same quantity
  with less variance and O(F) storage.  The spatial covariance is the identity -- the taps are drawn
  i.i.d. per antenna (synth_ref.py:213-217) -- so the ``s`` stage of the reference's order
  ``"s-f-t"`` is a no-op here and is left out.
* **Exact 2-D filter.**  Sionna's ``LMMSEInterpolator`` filters sequentially ("f-t"), which
  approximates the 2-D Wiener filter.  Here the estimate is the exact filter under the separable
  covariance ``R_t (x) R_f``, in an eigen form of ``R_t[D, D]`` that costs ``nd`` frequency GEMMs
  (``lmmse_design``), on the full band up to 3300 subcarriers (the reference splits grids above
  100 PRB into blocks).  The baseline is therefore, if anything, stronger than the reference's.
* **Scalar err_var.**  Sionna hands the detector a per-RE error variance; ``nrx_lmmse_detect`` takes
  one scalar.  ``EstimatorBaselineReceiver`` passes ``num_active x`` the mean of the theoretical
  error map over the data symbols (lmmse), or ``num_active * no / 2`` as ``baseline_lsnn_lmmse``
  does (lin).  Both are approximations of the per-RE quantity.
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Optional

import numpy as np

from . import _lib
from .baseline import MAX_TX, LMMSEDetector
from .generator import NUM_SYMBOLS, GenParams, SlotBatch

SYSTEMS = ("baseline_lslin_lmmse", "baseline_lmmse_lmmse")
KINDS = ("lin", "lmmse")
COV_SLOT_OFFSET = 1 << 40        # covariance slots start here: disjoint from every Monte-Carlo offset


def _torch():
    import torch
    return torch


def toeplitz(lags: np.ndarray) -> np.ndarray:
    """Hermitian Toeplitz R[i, j] = lags[i - j] (i >= j), conj(lags[j - i]) (i < j)."""
    lags = np.asarray(lags, np.complex128)
    n = len(lags)
    d = np.arange(n)[:, None] - np.arange(n)[None, :]
    return np.where(d >= 0, lags[np.abs(d)], np.conj(lags[np.abs(d)]))


def pilot_subcarriers(num_subcarriers: int, group: int) -> np.ndarray:
    return np.arange(group, num_subcarriers, 2)


class CovarianceEstimator:
    """Frequency and time covariance of the generator's channel from its true ``h``
    (``SlotGenerator(want_h=True)``): ``accumulate(sb)`` adds a batch's lag sums on the device
    (``nrx_cov_accumulate``, float64, deterministic), ``matrices()`` divides by the product counts
    and returns the Hermitian Toeplitz ``(R_f [F, F], R_t [14, 14])`` as numpy complex128.  The
    spatial covariance is the identity (module docstring), so there is no ``R_s``."""

    def __init__(self, params: GenParams, device: int = 0):
        torch = _torch()
        self.p = params
        self.device = device
        self._lib = _lib.load()
        self.acc = torch.zeros((params.num_subcarriers + NUM_SYMBOLS, 2), dtype=torch.float64,
                               device=f"cuda:{device}")
        self.slots = 0
        self._ws = None

    def accumulate(self, sb: SlotBatch, stream=None) -> None:
        torch = _torch()
        h = sb.h
        if h is None:
            raise ValueError("the covariance needs the true channel: SlotGenerator(want_h=True)")
        p = self.p
        B = h.shape[0]
        if tuple(h.shape) != (B, p.num_tx, p.num_subcarriers, NUM_SYMBOLS, 2 * p.num_rx_ant) \
                or h.dtype != torch.float32 or not h.is_contiguous() or h.device != self.acc.device:
            raise ValueError("h must be a contiguous float32 [B, U, F, 14, 2A] tensor on the estimator's device")
        io = _lib.nrx_cov_io()
        io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = B, p.num_tx, p.num_subcarriers, NUM_SYMBOLS
        io.num_rx_ant = p.num_rx_ant
        io.h, io.acc = h.data_ptr(), self.acc.data_ptr()
        n = ctypes.c_size_t()
        _lib.check(self._lib.nrx_cov_workspace_size(ctypes.byref(io), ctypes.byref(n)))
        if self._ws is None or self._ws.numel() < n.value:
            self._ws = torch.empty(n.value, dtype=torch.uint8, device=self.acc.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.acc.device).cuda_stream
        _lib.check(self._lib.nrx_cov_accumulate(ctypes.byref(io), self._ws.data_ptr(), self._ws.numel(), stream))
        self.slots += B

    def lags(self):
        """(r_f [F], r_t [14]) complex128: the lag sums over their product counts"""
        if not self.slots:
            raise ValueError("no slots accumulated")
        p = self.p
        F, T = p.num_subcarriers, NUM_SYMBOLS
        a = self.acc.cpu().numpy()
        s = a[:, 0] + 1j * a[:, 1]
        n = self.slots * p.num_tx * p.num_rx_ant
        return s[:F] / (n * T * (F - np.arange(F))), s[F:] / (n * F * (T - np.arange(T)))

    def matrices(self):
        r_f, r_t = self.lags()
        return toeplitz(r_f), toeplitz(r_t)


@dataclasses.dataclass
class LMMSEDesign:
    """Tables of ``nrx_chest_lmmse`` (include/nrx.h) and the theoretical error variance."""
    filt: np.ndarray        # [2, nd, F, Pmax, 2] f32: W_k of CDM group 0 / 1 (re, im)
    tcoef: np.ndarray       # [nd, 14, 2] f32: a_k[t]
    vconj: np.ndarray       # [nd, nd, 2] f32: conj(v_k[d])
    err_var: np.ndarray     # [2, F, 14] f64: E |h - h^|^2 per RE of a user of CDM group 0 / 1
    no: float


def lmmse_design(R_f: np.ndarray, R_t: np.ndarray, params: GenParams, no: float, dtype=np.float32) -> LMMSEDesign:
    """The exact 2-D Wiener filter under ``R_t (x) R_f`` for LS estimates at the own pilots
    ``P = {f : f mod 2 = group}`` of the DMRS symbols ``D`` with noise ``sigma^2 = no / 2`` (the
    generator's pilots have energy 2), in the eigen form of ``R_t[D, D] = V diag(lambda) V^H``:

        W_k = R_f[:, P] (R_f[P, P] + (sigma^2 / lambda_k) I)^-1,    a_k[t] = R_t[t, D] v_k / lambda_k
        h^[f, t] = sum_k a_k[t] (W_k z_k)[f],                       z_k = sum_d conj(v_k[d]) h_ls[P, D_d]

    which equals ``(R_t[:, D] (x) R_f[:, P]) (R_t[D, D] (x) R_f[P, P] + sigma^2 I)^-1`` (checked
    against that brute-force form in tests/test_chest_ref.py).  ``R_t`` is scaled to a unit diagonal
    first, so the prior variance of an RE is ``R_f[0, 0]`` (both matrices estimate the same power).
    The error map is ``e[f, t] = R_f[0, 0] - sum_j W_ij conj(C_ij)`` with ``C = R_t[:, D] (x) R_f[:, P]``,
    from the unrounded filter.  Components with ``lambda_k <= 1e-12 lambda_max`` are dropped (zero
    tables).  The tables are rounded once to float32, the kernel's format (``dtype=np.float64``
    keeps them unrounded, for checks)."""
    if not no > 0:
        raise ValueError("no must be > 0")
    F, T = params.num_subcarriers, NUM_SYMBOLS
    D = list(params.dmrs_symbols)
    nd = len(D)
    R_f = np.asarray(R_f, np.complex128)
    R_t = np.asarray(R_t, np.complex128)
    if R_f.shape != (F, F) or R_t.shape != (T, T):
        raise ValueError(f"R_f must be {(F, F)} and R_t {(T, T)}")
    R_t = R_t / R_t[0, 0].real
    sigma2 = float(no) / 2.0
    lam, V = np.linalg.eigh(R_t[np.ix_(D, D)])
    Pmax = (F + 1) // 2
    filt = np.zeros((2, nd, F, Pmax), np.complex128)
    tcoef = np.zeros((nd, T), np.complex128)
    vconj = np.zeros((nd, nd), np.complex128)
    err = np.full((2, F, T), R_f[0, 0].real)
    for k in range(nd):
        if lam[k] <= 1e-12 * lam[-1]:
            continue
        v = V[:, k]
        tcoef[k] = (R_t[:, D] @ v) / lam[k]
        vconj[k] = np.conj(v)
        for g in (0, 1):
            P = pilot_subcarriers(F, g)
            if not len(P):
                continue
            Rfp = R_f[:, P]
            W = np.linalg.solve(R_f[np.ix_(P, P)] + (sigma2 / lam[k]) * np.eye(len(P)), Rfp.conj().T).conj().T
            filt[g, k, :, :len(P)] = W
            q = np.real(np.sum(W * np.conj(Rfp), axis=1))                     # [F]
            err[g] -= lam[k] * q[:, None] * (np.abs(tcoef[k]) ** 2)[None, :]
    for g in (0, 1):
        if not len(pilot_subcarriers(F, g)):
            err[g] = R_f[0, 0].real
    ri = lambda z: np.ascontiguousarray(np.stack([z.real, z.imag], -1).astype(dtype))  # noqa: E731
    return LMMSEDesign(ri(filt), ri(tcoef), ri(vconj), err, float(no))


class ChannelEstimator:
    """``est(sb, no) -> h_est [B, U, F, 14, 2A]``: ``"lin"`` (``nrx_chest_lin``) or ``"lmmse"``
    (``nrx_chest_lmmse``) on the LS estimates that ``sb.h_hat`` holds at the own pilots.
    ``"lmmse"`` needs the covariance (``R_f``, ``R_t`` here or ``set_covariance``) and designs its
    filter whenever ``no`` changes (``self.design``); ``tables=`` pins given ``LMMSEDesign`` tables
    instead.  Every element of the output is written; inactive users are 0."""

    def __init__(self, kind: str, params: GenParams, device: int = 0, R_f=None, R_t=None,
                 tables: Optional[LMMSEDesign] = None):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        self.kind = kind
        self.p = params
        self.device = device
        self._lib = _lib.load()
        self.R_f, self.R_t = R_f, R_t
        self.design: Optional[LMMSEDesign] = None
        self._pinned = tables is not None
        self._dev = None
        self._out = None
        if tables is not None:
            self._set_design(tables)

    def set_covariance(self, R_f, R_t) -> None:
        self.R_f, self.R_t = R_f, R_t
        if not self._pinned:
            self.design = None

    def _set_design(self, d: LMMSEDesign) -> None:
        p = self.p
        nd, F = len(p.dmrs_symbols), p.num_subcarriers
        if d.filt.shape != (2, nd, F, (F + 1) // 2, 2) or d.tcoef.shape != (nd, NUM_SYMBOLS, 2) \
                or d.vconj.shape != (nd, nd, 2) or any(a.dtype != np.float32 for a in (d.filt, d.tcoef, d.vconj)):
            raise ValueError("tables do not match the parameters (lmmse_design)")
        self.design = d
        self._dev = None            # uploaded by the next call

    def prepare(self, no: float) -> Optional[LMMSEDesign]:
        """(re-)design the LMMSE filter for ``no``; the design in use"""
        if self.kind != "lmmse" or self._pinned:
            return self.design
        if self.design is None or self.design.no != float(no):
            if self.R_f is None or self.R_t is None:
                raise ValueError("the LMMSE estimator needs the covariance matrices (set_covariance)")
            self._set_design(lmmse_design(self.R_f, self.R_t, self.p, no))
        return self.design

    def __call__(self, sb: SlotBatch, no: float, out=None, stream=None):
        torch = _torch()
        p = self.p
        hh = sb.h_hat
        if hh is None:
            raise ValueError("the slot batch has no h_hat")
        B = hh.shape[0]
        shape = (B, p.num_tx, p.num_subcarriers, NUM_SYMBOLS, 2 * p.num_rx_ant)
        if tuple(hh.shape) != shape or hh.dtype != torch.float32 or not hh.is_contiguous() \
                or hh.device != torch.device(f"cuda:{self.device}"):
            raise ValueError(f"h_hat must be a contiguous float32 {shape} tensor on cuda:{self.device}")
        if tuple(sb.active.shape) != (B, p.num_tx) or sb.active.dtype != torch.float32 \
                or not sb.active.is_contiguous():
            raise ValueError(f"active must be a contiguous float32 {(B, p.num_tx)} tensor")
        if out is None:
            if self._out is None or self._out.shape[0] != B:
                self._out = torch.empty(shape, dtype=torch.float32, device=hh.device)
            out = self._out
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 {shape} tensor")
        io = _lib.nrx_chest_io()
        io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = shape[:4]
        io.num_rx_ant, io.num_dmrs_symbols = p.num_rx_ant, len(p.dmrs_symbols)
        for k, t in enumerate(list(p.dmrs_symbols)[:4]):
            io.dmrs_symbols[k] = t
        for u in range(min(p.num_tx, 16)):
            io.cdm_group[u] = p.cdm_group[u]
        io.no = float(no)
        io.h_hat, io.active, io.h_out = hh.data_ptr(), sb.active.data_ptr(), out.data_ptr()
        if stream is None:
            stream = torch.cuda.current_stream(hh.device).cuda_stream
        if self.kind == "lmmse":
            d = self.prepare(no)
            if self._dev is None:
                self._dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(hh.device)
                                  for a in (d.filt, d.tcoef, d.vconj))
            io.filt, io.tcoef, io.vconj = (t.data_ptr() for t in self._dev)
            _lib.check(self._lib.nrx_chest_lmmse(ctypes.byref(io), stream))
        else:
            _lib.check(self._lib.nrx_chest_lin(ctypes.byref(io), stream))
        return out


class EstimatorBaselineReceiver:
    """``rx(sb, no) -> llr [1, B, U, F, T, bits_max]`` for ``baseline_lslin_lmmse`` (linear
    interpolation) and ``baseline_lmmse_lmmse`` (2-D LMMSE estimation; needs ``R_f`` / ``R_t`` from
    a ``CovarianceEstimator``, here or through ``set_covariance``), both followed by the LMMSE
    detector of ``baseline.LMMSEDetector``.  Same call signature and ``contaminated`` property as
    ``baseline.BaselineReceiver``, and the same limit: both work on LS estimates at the pilots, so
    they are meaningful for at most one active port per CDM group.

    The detector takes one scalar ``err_var`` where Sionna passes a per-RE map -- an approximation
    in both systems: lmmse passes ``num_active x`` the mean over users' groups, subcarriers and data
    symbols of the theoretical error map of the design; lin passes ``num_active * no / 2``, the LS
    error at a pilot, as ``baseline_lsnn_lmmse`` does."""

    perfect_csi = False
    SYSTEMS = SYSTEMS

    def __init__(self, system: str, params: GenParams, device: int = 0, R_f=None, R_t=None):
        if system not in SYSTEMS:
            raise ValueError(f"system must be one of {SYSTEMS}, got {system!r}")
        if params.num_tx > MAX_TX:
            raise ValueError(f"the LMMSE kernel is built for at most {MAX_TX} users, got {params.num_tx}")
        self.system = system
        self.p = params
        self.estimator = ChannelEstimator("lmmse" if system == "baseline_lmmse_lmmse" else "lin", params, device,
                                          R_f=R_f, R_t=R_t)
        self.detector = LMMSEDetector(device)
        self._out = None
        self.last_h = None      # the estimate the last call detected with

    def set_covariance(self, R_f, R_t) -> None:
        self.estimator.set_covariance(R_f, R_t)

    @property
    def _num_active(self) -> int:
        return self.p.num_tx if self.p.num_active is None else self.p.num_active

    @property
    def contaminated(self) -> bool:
        """the LS estimates can be pilot-contaminated: two active ports may share a CDM group"""
        groups = list(self.p.cdm_group[:self.p.num_tx])
        return self._num_active > 1 and max(groups.count(g) for g in set(groups)) > 1

    def err_var(self, no: float) -> float:
        if self.estimator.kind == "lin":
            return self._num_active * float(no) / 2.0
        d = self.estimator.prepare(no)
        data = [t for t in range(NUM_SYMBOLS) if t not in self.p.dmrs_symbols]
        groups = list(self.p.cdm_group[:self.p.num_tx])
        return self._num_active * float(np.mean([d.err_var[g][:, data].mean() for g in groups]))

    def __call__(self, sb: SlotBatch, no: float, out=None, stream=None):
        p = self.p
        ev = self.err_var(no)
        h = self.last_h = self.estimator(sb, no, stream=stream)
        if out is None:
            B = h.shape[0]
            if self._out is None or self._out.shape[1] != B:
                torch = _torch()
                self._out = torch.empty((1, B, p.num_tx, p.num_subcarriers, NUM_SYMBOLS, p.bits_max),
                                        dtype=torch.float32, device=h.device)
            out = self._out
        return self.detector(sb.y, h, sb.active, sb.mcs, p.mcs_bits, no, p.dmrs_symbols, err_var=ev, out=out,
                             stream=stream)


def estimate_covariance(gen, num_slots: int, batch_size: int, no: float = 1.0,
                        slot_offset: int = COV_SLOT_OFFSET) -> CovarianceEstimator:
    """Accumulate the covariance over ``num_slots`` generated slots starting at ``slot_offset``
    (default 2^40, beyond every Monte-Carlo offset), as the reference runs compute_cov_mat.py before
    an evaluation.  The true channel does not depend on ``no``.  ``gen`` needs ``want_h=True``."""
    if not gen.want_h:
        raise ValueError("the covariance needs SlotGenerator(want_h=True)")
    cov = CovarianceEstimator(gen.p, gen.device)
    done = 0
    while done < num_slots:
        b = min(batch_size, num_slots - done)
        cov.accumulate(gen(b, no, slot_offset=slot_offset + done))
        done += b
    return cov
