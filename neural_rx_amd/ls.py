"""Cover-coded DMRS ports and the despreading least-squares channel estimator on the GPU.

The receiver-side step that turns a received grid ``y`` and the known pilot sequence into the
``h_hat`` that ``NeuralReceiver`` / ``nrx_forward`` (and, as the Aerial pilot list,
``nrx_forward_aerial``) consume -- the reference's ``NeuralPUSCHReceiver.estimate_channel``
(neural_rx.py:1462-1514).  The device work is ``nrx_ls_estimate`` of ``libnrx.so`` (include/nrx.h,
csrc/nrx_ls.hip); torch tensors are only device containers and a missing library is an error.
The slot generator uses the same device code for its own ``h_hat`` (``GenParams.dmrs``).

``DMRSPorts`` holds the ports: port u is (``cdm_group[u]``, ``focc[u]``, ``tocc[u]``) -- the comb
offset, a frequency cover over pairs of comb positions and a time cover over pairs of DMRS symbols,
eight orthogonal ports in all.  ``DMRSPorts.default(U)`` is this project's assignment rule, the
arrangement of DMRS configuration type 1: ``g = (u >> 1) & 1``, ``wf = u & 1``, ``wt = (u >> 2) & 1``.
The base sequence is the project's own seeded QPSK, not the Gold sequence of TS 38.211
(tests/dmrs_ref.py states ports, sequence and estimator in numpy).
"""
from __future__ import annotations

import dataclasses
from typing import Sequence

from . import _lib
from ._call import fill_dmrs, fill_grid, ptr, ref, require, stream_of, torch as _torch

NUM_SYMBOLS = 14
MAX_PORTS = 8       # 2 CDM groups x 2 frequency covers x 2 time covers


@dataclasses.dataclass(frozen=True)
class DMRSPorts:
    """The (cdm_group, focc, tocc) of ``num_tx`` ports.  ``despread_f`` / ``despread_t``: whether an
    estimator for these ports has to average the frequency / time pair, i.e. whether any port in
    use carries that cover."""
    cdm_group: Sequence[int]
    focc: Sequence[int]
    tocc: Sequence[int]

    def __post_init__(self):
        for name in ("cdm_group", "focc", "tocc"):
            object.__setattr__(self, name, tuple(int(v) for v in getattr(self, name)))
        n = len(self.cdm_group)
        if not 1 <= n <= 16 or len(self.focc) != n or len(self.tocc) != n:
            raise ValueError("cdm_group, focc and tocc need one entry per port, 1..16 ports")
        if any(v not in (0, 1) for v in self.cdm_group + self.focc + self.tocc):
            raise ValueError("cdm_group, focc and tocc must be 0/1")
        ports = list(zip(self.cdm_group, self.focc, self.tocc))
        if len(set(ports)) != n:
            raise ValueError("two ports share one (cdm_group, focc, tocc)")

    @classmethod
    def from_ports(cls, ports: Sequence[int]) -> "DMRSPorts":
        """the ports with these numbers (0..7) under the project's rule (module docstring); ports
        [0, 2] are the two uncovered ports of the two CDM groups"""
        ports = [int(i) for i in ports]
        if any(not 0 <= i < MAX_PORTS for i in ports):
            raise ValueError(f"there are {MAX_PORTS} orthogonal ports, numbered 0..{MAX_PORTS - 1}; got {ports}")
        return cls([(i >> 1) & 1 for i in ports], [i & 1 for i in ports], [(i >> 2) & 1 for i in ports])

    @classmethod
    def default(cls, num_tx: int) -> "DMRSPorts":
        """ports 0..num_tx-1; at most 8"""
        if not 1 <= num_tx <= MAX_PORTS:
            raise ValueError(f"there are {MAX_PORTS} orthogonal ports, got num_tx = {num_tx}")
        return cls.from_ports(range(num_tx))

    @classmethod
    def for_config(cls, cfg, num_tx: int) -> "DMRSPorts":
        """the first ports are the config's own (``dmrs_port_sets``, first port of each set: 0 and 2 for
        the two-user configs, whose ports stay what the shipped weights were trained on); further
        users take the lowest port numbers not yet in use"""
        if not 1 <= num_tx <= MAX_PORTS:
            raise ValueError(f"there are {MAX_PORTS} orthogonal ports, got num_tx = {num_tx}")
        ports = [int(s[0]) for s in cfg.dmrs_port_sets][:num_tx]
        ports += [i for i in range(MAX_PORTS) if i not in ports][:num_tx - len(ports)]
        return cls.from_ports(ports)

    @property
    def num_tx(self) -> int:
        return len(self.cdm_group)

    @property
    def despread_f(self) -> bool:
        return any(self.focc)

    @property
    def despread_t(self) -> bool:
        return any(self.tocc)

    @property
    def block(self) -> int:
        """pilots averaged per estimate: 1, 2 or 4"""
        return (2 if self.despread_f else 1) * (2 if self.despread_t else 1)

    def validate(self, num_subcarriers: int, dmrs_symbols: Sequence[int]) -> None:
        """the grid rules of nrx_ls_estimate (include/nrx.h), as ValueError"""
        if self.despread_f and num_subcarriers % 4:
            raise ValueError("a frequency cover needs num_subcarriers % 4 == 0 (pairs of comb positions)")
        d = list(dmrs_symbols)
        if self.despread_t and (len(d) % 2 or any(d[k + 1] != d[k] + 1 for k in range(0, len(d) - 1, 2))):
            raise ValueError(f"a time cover needs DMRS symbols in pairs (t, t + 1), e.g. 2 3 10 11; got {d}")


class LSEstimator:
    """``est(y, pilots, active=None) -> h_hat`` (``aerial=True``: ``(h_hat, h_ls_real, h_ls_imag)``)
    through ``nrx_ls_estimate``.  ``y [B, F, 14, 2A]``, ``pilots [2, Pmax, nd, 2]`` (the base sequence
    of the two CDM groups, any non-zero values; ``SlotBatch.pilots`` of the generator) and ``active
    [B, U]`` are contiguous float32 device tensors; the outputs are the estimator's own buffers,
    reused by the next call of the same batch size."""

    def __init__(self, ports: DMRSPorts, num_subcarriers: int, num_rx_ant: int, dmrs_symbols: Sequence[int],
                 aerial: bool = False, device: int = 0):
        ports.validate(num_subcarriers, dmrs_symbols)
        self.ports = ports
        self.F, self.A = int(num_subcarriers), int(num_rx_ant)
        self.dmrs_symbols = [int(t) for t in dmrs_symbols]
        self.aerial = aerial
        self.device = device
        self._lib = _lib.load()
        self._out = None

    def io(self, batch: int) -> _lib.nrx_ls_io:
        p = self.ports
        io = _lib.nrx_ls_io()
        fill_grid(io, batch, p.num_tx, self.F, NUM_SYMBOLS, self.A)
        fill_dmrs(io, self.dmrs_symbols, p.cdm_group, p.num_tx)
        for u in range(p.num_tx):       # DMRSPorts holds at most 16
            io.focc[u], io.tocc[u] = p.focc[u], p.tocc[u]
        io.despread_f, io.despread_t = int(p.despread_f), int(p.despread_t)
        return io

    def __call__(self, y, pilots, active=None, stream=None):
        torch = _torch()
        B, U, F, A, nd = y.shape[0], self.ports.num_tx, self.F, self.A, len(self.dmrs_symbols)
        want = {"y": (y, (B, F, NUM_SYMBOLS, 2 * A)), "pilots": (pilots, (2, (F + 1) // 2, nd, 2))}
        if active is not None:
            want["active"] = (active, (B, U))
        if not y.is_cuda:
            raise ValueError("y must be on the GPU")
        for name, (t, shape) in want.items():
            require(name, t, shape, torch.float32, y.device)
        if self._out is None or self._out[0].shape[0] != B or self._out[0].device != y.device:
            f32 = dict(dtype=torch.float32, device=y.device)
            out = [torch.empty((B, U, F, NUM_SYMBOLS, 2 * A), **f32)]
            if self.aerial:
                out += [torch.empty((B, nd * (F // 2), U, A), **f32) for _ in range(2)]
            self._out = out
        io = self.io(B)
        io.y, io.pilots, io.active, io.h_hat = ptr(y), ptr(pilots), ptr(active), ptr(self._out[0])
        if self.aerial:
            io.h_ls_real, io.h_ls_imag = ptr(self._out[1]), ptr(self._out[2])
        _lib.check(self._lib.nrx_ls_estimate(ref(io), stream_of(y, stream)))
        return tuple(self._out) if self.aerial else self._out[0]
