"""OFDM modulation and demodulation on the GPU: the step between time-domain I/Q samples and the resource
grid that ``NeuralReceiver``, ``ls.LSEstimator`` and the baselines consume.

``OFDMModulator(cyclic_prefix_length)`` and ``OFDMDemodulator(fft_size, l_min, cyclic_prefix_length)`` carry
the names and the argument order of the reference's layers (utils/siona_tf.py:4407-4643; unitary transforms,
4331-4402).  The device work is ``nrx_ofdm_modulate`` / ``nrx_ofdm_demodulate`` of ``libnrx.so`` (include/nrx.h,
csrc/nrx_ofdm.hip): one launch each, the transform in LDS between its one read and its one write.  Torch
tensors are only device containers and a missing library is an error.

Tensors.  ``samples [B, S, L]`` complex (complex64 for ``precision="f32"``, complex128 for ``"f64"``).  The grid,
by ``layout``: ``"planar"`` ``[B, S, F, T]`` complex, or ``"cgnn"`` ``[B, F, T, 2S]`` real (``nrx_io.y``: S the
receive antennas).  ``num_subcarriers`` F <= N grid subcarriers sit at ``first_bin`` of the fftshifted axis
(default: centred); the reference's layers are F = N, ``first_bin = 0``.  ``cyclic_prefix_length`` is one int or
one per symbol (``default_cp(N)``: the normal cyclic prefix of NR).

A receive path from samples, for a CGNN engine ``rx`` and its ``ls.LSEstimator`` ``est``::

    demod = OFDMDemodulator(4096, 0, default_cp(4096), num_subcarriers=F, layout="cgnn")
    y = demod(samples)                      # [B, A, L] complex64 -> [B, F, 14, 2A] float32
    h_hat = est(y, pilots, active)
    llr = rx(y, h_hat, active)
"""
from __future__ import annotations

from typing import Optional, Sequence

from . import _lib
from ._call import ptr, ref, require, stream_of, torch as _torch

NUM_SYMBOLS = 14


def default_cp(fft_size: int) -> int:
    """``9 N // 128``: 288 at N = 4096, the normal cyclic prefix of NR"""
    return 9 * int(fft_size) // 128


def rapp(asat: float, p: float = 2.0) -> tuple:
    """the Rapp power-amplifier curve ``v / (1 + (|v| / asat)^(2p))^(1 / (2p))`` as the modulator's ``pa=``"""
    if not asat > 0 or not p > 0:
        raise ValueError("rapp needs asat > 0 and p > 0")
    return float(asat), float(p)


def _cp_list(cp, T: int) -> list:
    v = [int(c) for c in (cp if isinstance(cp, (list, tuple)) else [cp])]
    if len(v) == 1:
        v = v * T
    if len(v) != T:
        raise ValueError(f"cyclic_prefix_length needs one value or one per symbol: {T}, got {len(v)}")
    return v


class _Ofdm:
    def __init__(self, cyclic_prefix_length, fft_size, num_subcarriers, first_bin, layout, precision,
                 num_symbols):
        if layout not in _lib.OFDM_LAYOUTS or precision not in _lib.OFDM_PRECISIONS:
            raise ValueError(f"layout must be one of {tuple(_lib.OFDM_LAYOUTS)} and precision one of "
                             f"{tuple(_lib.OFDM_PRECISIONS)}")
        self.cyclic_prefix_length = cyclic_prefix_length
        self.fft_size = None if fft_size is None else int(fft_size)
        self.num_subcarriers = num_subcarriers
        self.first_bin, self.layout, self.precision = int(first_bin), layout, precision
        self.num_symbols = int(num_symbols)
        self._lib = _lib.load()

    def _dtypes(self):
        torch = _torch()
        return ((torch.complex64, torch.float32) if self.precision == "f32" else (torch.complex128, torch.float64))

    def num_samples(self, fft_size: Optional[int] = None) -> int:
        """samples of the ``num_symbols`` symbols with their prefixes"""
        N = self.fft_size if fft_size is None else fft_size
        return sum(c + N for c in _cp_list(self.cyclic_prefix_length, self.num_symbols))

    def _io(self, B, S, F, T, N, L) -> _lib.nrx_ofdm_io:
        io = _lib.nrx_ofdm_io()
        io.batch, io.num_streams, io.grid_subcarriers, io.num_symbols = B, S, F, T
        io.fft_size, io.first_bin = N, self.first_bin
        for t, c in enumerate(_cp_list(self.cyclic_prefix_length, T)[:14]):
            io.cp_length[t] = c
        io.precision, io.grid_layout = _lib.OFDM_PRECISIONS[self.precision], _lib.OFDM_LAYOUTS[self.layout]
        io.num_samples = L
        return io

    def _grid_shape(self, B, S, F, T):
        return (B, S, F, T) if self.layout == "planar" else (B, F, T, 2 * S)

    def _grid_dims(self, grid):
        """(B, S, F, T) of a grid tensor in this layout"""
        if grid.dim() != 4:
            raise ValueError(f"grid must have 4 dimensions, got {tuple(grid.shape)}")
        if self.layout == "planar":
            return tuple(grid.shape)
        B, F, T, S2 = grid.shape
        return B, S2 // 2, F, T


class OFDMModulator(_Ofdm):
    """``mod(grid) -> samples [B, S, L]``.  ``fft_size`` defaults to the grid's F (the reference's layer); ``pa``:
    ``rapp(asat, p)``, the amplifier curve applied at the store; ``num_samples``: L, at least the symbols with
    their prefixes (the rest is written zero)."""

    def __init__(self, cyclic_prefix_length=0, *, fft_size: Optional[int] = None, first_bin: int = -1,
                 layout: str = "planar", precision: str = "f32", pa: Optional[tuple] = None,
                 num_samples: Optional[int] = None):
        super().__init__(cyclic_prefix_length, fft_size, None, first_bin, layout, precision, NUM_SYMBOLS)
        self.pa = pa
        self.L = num_samples

    def __call__(self, grid, out=None, stream=None):
        torch = _torch()
        cdt, rdt = self._dtypes()
        if not grid.is_cuda:
            raise ValueError("grid must be on the GPU")
        B, S, F, T = self._grid_dims(grid)
        require("grid", grid, self._grid_shape(B, S, F, T), cdt if self.layout == "planar" else rdt)
        N = self.fft_size or F
        self.num_symbols = T
        L = self.L if self.L is not None else self.num_samples(N)
        if out is None:
            out = torch.empty((B, S, L), dtype=cdt, device=grid.device)
        require("out", out, (B, S, L), cdt, grid.device)
        io = self._io(B, S, F, T, N, L)
        if self.pa is not None:
            io.pa_asat, io.pa_smoothness = self.pa
        io.grid, io.samples = ptr(grid), ptr(out)
        _lib.check(self._lib.nrx_ofdm_modulate(ref(io), stream_of(grid, stream)))
        return out


class OFDMDemodulator(_Ofdm):
    """``demod(samples [B, S, L]) -> grid``.  ``l_min <= 0`` as in the reference: the windows start ``-l_min``
    samples early and the phase ramp of that advance is removed.  ``offset``: one int or one per stream, added
    to every window start (samples outside the row read as zero); ``num_symbols``: T, 1..14."""

    def __init__(self, fft_size: int, l_min: int = 0, cyclic_prefix_length=0, *, num_subcarriers: Optional[int] = None,
                 first_bin: int = -1, layout: str = "planar", precision: str = "f32", offset=0,
                 num_symbols: int = NUM_SYMBOLS):
        super().__init__(cyclic_prefix_length, fft_size, num_subcarriers, first_bin, layout, precision, num_symbols)
        if l_min > 0:
            raise ValueError("l_min must be nonpositive")
        self.l_min = int(l_min)
        self.offset = offset

    def _offsets(self, S) -> Sequence[int]:
        v = [int(o) for o in (self.offset if isinstance(self.offset, (list, tuple)) else [self.offset])]
        if len(v) == 1:
            v = v * S
        if len(v) != S:
            raise ValueError(f"offset needs one value or one per stream: {S}, got {len(v)}")
        return v

    def __call__(self, samples, out=None, stream=None):
        torch = _torch()
        cdt, rdt = self._dtypes()
        if not samples.is_cuda:
            raise ValueError("samples must be on the GPU")
        if samples.dim() != 3:
            raise ValueError(f"samples must be [B, S, L], got {tuple(samples.shape)}")
        B, S, L = samples.shape
        require("samples", samples, (B, S, L), cdt)
        N, T = self.fft_size, self.num_symbols
        F = N if self.num_subcarriers is None else int(self.num_subcarriers)
        shape = self._grid_shape(B, S, F, T)
        gdt = cdt if self.layout == "planar" else rdt
        if out is None:
            out = torch.empty(shape, dtype=gdt, device=samples.device)
        require("out", out, shape, gdt, samples.device)
        io = self._io(B, S, F, T, N, L)
        io.timing_advance = -self.l_min
        for s, o in enumerate(self._offsets(S)[:16]):
            io.offset[s] = o
        io.grid, io.samples = ptr(out), ptr(samples)
        _lib.check(self._lib.nrx_ofdm_demodulate(ref(io), stream_of(samples, stream)))
        return out
