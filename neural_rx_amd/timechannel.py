"""The time-domain channel on the GPU: per-sample Doppler and fractional-delay taps on the samples between
``ofdm.OFDMModulator`` and ``ofdm.OFDMDemodulator`` -- the counterpart of Sionna's ``TimeChannel``.

``TimeChannel(sample_rate, l_min, l_max, n0)`` is the thin wrapper of ``nrx_time_channel`` of ``libnrx.so``
(include/nrx.h, csrc/nrx_timechan.hip): one launch, float64, no workspace.  With fs the sample rate::

    r[b,a,n] = sum_u sum_l g[b,u,a,l](n) v[b,u,l](n)
    g(n)     = sum_s g0[b,u,a,l,s] exp(j 2 pi fd[b,u,a,l,s] (n - n0) / fs)
    v(n)     = sum_{l'=l_min..l_max} sinc(l' - tau[b,u,l] fs) x[b,u,n - l']        (x = 0 outside the row)

The sinc is plainly truncated to ``l_min..l_max`` (no window, no re-normalisation), so a path's energy is
preserved only approximately.  Torch tensors are only device containers and a missing library is an error.

Tensors: ``x [B, U, Ls]`` complex128, ``tau [B, U, L]`` float64 (seconds), ``g0 [B, U, A, L, NS]`` complex128,
``fd [B, U, A, L, NS]`` float64 (Hz), ``rx_mix [A, A]`` complex128 or None; the result ``r [B, A, Ls]`` complex128.
"""
from __future__ import annotations

from . import _lib
from ._call import ptr, ref, require, stream_of, torch as _torch


class TimeChannel:
    """``chan(x, tau, g0, fd, rx_mix=None) -> r``"""

    def __init__(self, sample_rate: float, l_min: int = -6, l_max: int = 6, n0: int = 0):
        self.sample_rate, self.l_min, self.l_max, self.n0 = float(sample_rate), int(l_min), int(l_max), int(n0)
        self._lib = _lib.load()

    def __call__(self, x, tau, g0, fd, rx_mix=None, out=None, stream=None):
        torch = _torch()
        if not x.is_cuda:
            raise ValueError("x must be on the GPU")
        if x.dim() != 3 or g0.dim() != 5:
            raise ValueError(f"x must be [B, U, Ls] and g0 [B, U, A, L, NS], got {tuple(x.shape)} and {tuple(g0.shape)}")
        B, U, Ls = x.shape
        A, L, NS = g0.shape[2:]
        c128, f64, dev = torch.complex128, torch.float64, x.device
        require("x", x, (B, U, Ls), c128)
        require("tau", tau, (B, U, L), f64, dev)
        require("g0", g0, (B, U, A, L, NS), c128, dev)
        require("fd", fd, (B, U, A, L, NS), f64, dev)
        if rx_mix is not None:
            require("rx_mix", rx_mix, (A, A), c128, dev)
        if out is None:
            out = torch.empty((B, A, Ls), dtype=c128, device=dev)
        require("out", out, (B, A, Ls), c128, dev)
        io = _lib.nrx_tc_io()
        io.batch, io.num_tx, io.num_rx_ant, io.num_paths, io.num_sinusoids = B, U, A, L, NS
        io.l_min, io.l_max, io.num_samples, io.n0, io.sample_rate = self.l_min, self.l_max, Ls, self.n0, self.sample_rate
        io.tau, io.g0, io.fd, io.x, io.rx_mix, io.r = ptr(tau), ptr(g0), ptr(fd), ptr(x), ptr(rx_mix), ptr(out)
        _lib.check(self._lib.nrx_time_channel(ref(io), stream_of(x, stream)))
        return out
