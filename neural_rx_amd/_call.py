"""What every wrapper of ``libnrx.so`` does around its C call, stated once: the lazy torch import,
stream and pointer arguments, filling the descriptor fields that the ``*_io`` structs share
(``_lib.GRID`` / ``MCS`` / ``DMRS``), the tensor check and the workspace buffer.  Only helpers that at
least two wrappers use live here; everything is plain functions, cheap enough for the forward's
host path.
"""
from __future__ import annotations

import ctypes

from . import _lib


def torch():
    import torch
    return torch


def stream_of(where, stream):
    """``stream``, or the handle of the current stream of ``where`` (a tensor or a device) for None"""
    if stream is not None:
        return stream
    return torch().cuda.current_stream(getattr(where, "device", where)).cuda_stream


def ptr(t):
    """``t.data_ptr()``, None (a NULL pointer) for None"""
    return t.data_ptr() if t is not None else None


def ref(s):
    """``ctypes.byref(s)``, None (a NULL pointer) for None"""
    return ctypes.byref(s) if s is not None else None


# The fillers write at most what the C arrays hold and store the true counts, so an oversize argument
# reaches the C check and comes back as NRXError.
def fill_grid(io, B, U, F, T, A=None):
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = B, U, F, T
    if A is not None:
        io.num_rx_ant = A


def fill_mcs(io, mcs_bits, dmrs_symbols=None, bits_stride=None, num_heads=None):
    """``num_mcs`` / ``mcs_bits`` and, where given, the data-symbol mask (bit t set: symbol t carries
    DMRS), ``bits_stride`` and ``num_heads``"""
    io.num_mcs = len(mcs_bits)
    for m, b in enumerate(list(mcs_bits)[:8]):
        io.mcs_bits[m] = int(b)
    if dmrs_symbols is not None:
        mask = 0
        for t in dmrs_symbols:
            mask |= 1 << t
        io.dmrs_symbol_mask = mask
    if bits_stride is not None:
        io.bits_stride = bits_stride
    if num_heads is not None:
        io.num_heads = num_heads


def fill_dmrs(io, dmrs_symbols, cdm_group, num_tx):
    """``num_dmrs_symbols`` / ``dmrs_symbols`` and the CDM group of the first ``num_tx`` ports"""
    io.num_dmrs_symbols = len(dmrs_symbols)
    for k, t in enumerate(list(dmrs_symbols)[:4]):
        io.dmrs_symbols[k] = t
    for u in range(min(num_tx, 16)):
        io.cdm_group[u] = cdm_group[u]


def require(name, t, shape=None, dtype=None, device=None, contiguous=True):
    """The one tensor check: ValueError unless ``t`` has the shape, dtype and device asked for (None:
    any) and is contiguous."""
    if device is not None and not isinstance(device, torch().device):
        device = torch().device(device)
    if (shape is None or tuple(t.shape) == tuple(shape)) and (dtype is None or t.dtype == dtype) \
            and (device is None or t.device == device) and (not contiguous or t.is_contiguous()):
        return t
    want = " ".join(str(w) for w in ("contiguous" if contiguous else None, str(dtype)[6:] if dtype else None,
                                     tuple(shape) if shape is not None else None) if w is not None)
    raise ValueError(f"{name} must be a {want} tensor" + (f" on {device}" if device is not None else "")
                     + f", got {'' if t.is_contiguous() else 'non-contiguous '}{str(t.dtype)[6:]} "
                       f"{tuple(t.shape)} on {t.device}")


class Workspace:
    """A grow-only uint8 device buffer and the size query that goes with it.  ``buf`` is the cached
    tensor (None before the first ``get``)."""

    def __init__(self):
        self.buf = None
        self._sizes = {}

    def size(self, fn, *args, key=None) -> int:
        """what ``fn(*args, &bytes)`` asks for; with ``key``, asked once per key"""
        if key is not None and key in self._sizes:
            return self._sizes[key]
        n = ctypes.c_size_t()
        _lib.check(fn(*args, ctypes.byref(n)))
        if key is not None:
            self._sizes[key] = n.value
        return n.value

    def get(self, nbytes, device, given=None):
        """The caller's ``workspace=`` tensor, checked and passed on as it is (the C call checks its
        size: NRX_ERR_WORKSPACE when it is too small) -- or the cached buffer, allocated at exactly
        ``nbytes`` when it is missing, smaller or on another device."""
        t = torch()
        if not isinstance(device, t.device):
            device = t.device(device)
        if given is not None:
            if given.device != device or given.dtype != t.uint8 or not given.is_contiguous():
                raise ValueError(f"workspace must be a contiguous uint8 tensor on {device}")
            return given
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = t.empty(nbytes, dtype=t.uint8, device=device)
        return self.buf
