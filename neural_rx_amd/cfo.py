"""DMRS-based estimation and compensation of a carrier frequency offset on the GPU.

The receiver-side remedy for the generator's per-user CFO (``GenParams.cfo_hz``; the reference's
``cfo_offset_ppm(_eval)``, utils/impairments.py:18-110, has no counterpart of it).  The device
work is in ``libnrx.so`` (``nrx_cfo_estimate``, ``nrx_cfo_rotate``: include/nrx.h, csrc/nrx_cfo.hip);
torch tensors are only device containers and a missing library is an error.

``eps`` is the offset in subcarrier spacings.  The estimate is the phase of the correlation of the
own-pilot LS estimates of the closest DMRS symbol pair, so a Doppler shift common to a user's taps
is estimated (and compensated) with it; it is unambiguous for ``|eps| < 1 / (2 * 1.07 * gap)``.

* ``CFOCompensator.estimate(sb)``: ``eps_hat [B, U]`` float64.
* ``CFOCompensator.apply_nn(sb)``: the batch with the nearest-neighbour ``h_hat`` turned, symbol by
  symbol, to the phase it would have been estimated with at that symbol -- the input of the CGNN
  and of ``baseline_lsnn_lmmse``.
* ``CFOCompensator.wrap(estimator)``: de-rotate the pilots to symbol 0, run a
  ``chest.ChannelEstimator`` (whose interpolation then sees the channel without the rotation),
  re-rotate its output.  ``ChannelEstimator(..., cfo=comp)`` does this on every call.
"""
from __future__ import annotations

import dataclasses

from . import _lib
from ._call import fill_dmrs, fill_grid, ref, require, stream_of, torch as _torch
from .generator import NUM_SYMBOLS, GenParams, SlotBatch


class CFOCompensator:
    def __init__(self, params: GenParams, device: int = 0):
        if params.dmrs is not None and params.dmrs.despread_t:
            raise ValueError("the DMRS-based CFO estimate does not work on time-despread pilots (ports with a time "
                             "cover): the two symbols of a pair hold one estimate, so the closest pair shows no rotation")
        self.p = params
        self.device = device
        self._lib = _lib.load()
        self._eps = None
        self._nn = None
        self._pil = None

    def _io(self, h, eps) -> _lib.nrx_cfo_io:
        torch = _torch()
        p = self.p
        B = h.shape[0]
        shape = (B, p.num_tx, p.num_subcarriers, NUM_SYMBOLS, 2 * p.num_rx_ant)
        require("the channel tensor", h, shape, torch.float32, f"cuda:{self.device}")
        require("eps", eps, (B, p.num_tx), torch.float64, h.device)
        io = _lib.nrx_cfo_io()
        fill_grid(io, *shape[:4], p.num_rx_ant)
        fill_dmrs(io, p.dmrs_symbols, p.cdm_group, p.num_tx)
        io.h_in, io.eps = h.data_ptr(), eps.data_ptr()
        return io

    def estimate(self, sb: SlotBatch, out=None, stream=None):
        """``eps_hat [B, U]`` float64 from ``sb.h_hat`` at the own pilots; 0 for inactive users and
        with fewer than two DMRS symbols.  ``out=None`` returns the compensator's own buffer, which
        the next call overwrites."""
        torch = _torch()
        hh = sb.h_hat
        if hh is None:
            raise ValueError("the slot batch has no h_hat")
        B = hh.shape[0]
        if out is None:
            if self._eps is None or self._eps.shape[0] != B:
                self._eps = torch.empty((B, self.p.num_tx), dtype=torch.float64, device=hh.device)
            out = self._eps
        io = self._io(hh, out)
        require("active", sb.active, (B, self.p.num_tx), torch.float32)
        io.active = sb.active.data_ptr()
        _lib.check(self._lib.nrx_cfo_estimate(ref(io), stream_of(hh, stream)))
        return out

    def rotate(self, h, eps, ref_mode: int, sign: int, out=None, stream=None):
        """``out = h * exp(j * sign * 2 pi 1.07 eps (t - t_ref))`` (``nrx_cfo_rotate``); ``out=None``
        rotates in place."""
        io = self._io(h, eps)
        out = h if out is None else out
        require("out", out, h.shape, h.dtype, h.device)
        io.ref_mode, io.sign, io.h_out = int(ref_mode), int(sign), out.data_ptr()
        _lib.check(self._lib.nrx_cfo_rotate(ref(io), stream_of(h, stream)))
        return out

    def apply_nn(self, sb: SlotBatch, eps=None, stream=None) -> SlotBatch:
        """A copy of ``sb`` whose ``h_hat`` is the compensated nearest-neighbour estimate (a buffer
        of the compensator's, overwritten by the next call); ``sb`` itself is not touched.
        ``eps``: the offsets to compensate, default ``estimate(sb)``."""
        torch = _torch()
        if eps is None:
            eps = self.estimate(sb, stream=stream)
        if self._nn is None or self._nn.shape != sb.h_hat.shape:
            self._nn = torch.empty_like(sb.h_hat)
        h = self.rotate(sb.h_hat, eps, _lib.CFO_REF_NEAREST_DMRS, +1, out=self._nn, stream=stream)
        return dataclasses.replace(sb, h_hat=h)

    def wrap(self, estimator):
        """``est(sb, no, out=None, stream=None, workspace=None) -> h_est`` running ``estimator`` (a
        ``chest.ChannelEstimator``) between a de-rotation of the pilots to symbol 0 and the
        re-rotation of its output."""
        def est(sb: SlotBatch, no: float, out=None, stream=None, workspace=None):
            torch = _torch()
            eps = self.estimate(sb, stream=stream)
            if self._pil is None or self._pil.shape != sb.h_hat.shape:
                self._pil = torch.empty_like(sb.h_hat)
            pil = self.rotate(sb.h_hat, eps, _lib.CFO_REF_ZERO, -1, out=self._pil, stream=stream)
            h = estimator(dataclasses.replace(sb, h_hat=pil), no, out=out, stream=stream, workspace=workspace,
                          cfo=False)
            return self.rotate(h, eps, _lib.CFO_REF_ZERO, +1, stream=stream)
        return est
