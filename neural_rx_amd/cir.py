"""Channel impulse response (CIR) datasets and their replay in the slot generator.

The reference's second channel family, ``channel_type = "Dataset"`` (utils/channel_models.py:163-321): a
file of path coefficients ``a`` and path delays ``tau`` -- from a ray tracer, a measurement campaign or
another simulator -- from which an example is drawn per (slot, user).  Here the file is an ``.npz`` with
exactly the keys ``a`` (complex64 ``[E, A, L, Ta]``, Ta = 1 or 14) and ``tau`` (float32 ``[E, L]``, seconds),
and the replay is ``nrx_generate_slots_cir`` (include/nrx.h; tests/cir_ref.py states it in numpy):

    H_u[a, f, t] = sum_l a[e, a, l, t] exp(-j 2 pi (f + f_offset) subcarrier_spacing tau[e, l])

``GenParams(cir=CIRChannel(dataset, ...))`` routes a ``SlotGenerator`` through it; bits, noise, MCS and
active ports stay those of the built-in channel of the same seed, so curves on the two are paired.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

SELECT = {"index": 0, "random": 1, "trajectory": 2}
NUM_SYMBOLS = 14
MAX_EXAMPLES, MAX_PATHS = 1 << 24, 1024


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


class CIRDataset:
    """``a`` complex64 ``[E, A, L, Ta]``, ``tau`` float32 ``[E, L]`` -- numpy arrays, or torch tensors after
    ``to(device)``.  A padded path (all coefficients zero) with a non-finite or negative delay gets delay 0."""

    def __init__(self, a, tau):
        if _is_tensor(a):
            self.a, self.tau = a, tau
            shape_a, shape_t = tuple(a.shape), tuple(tau.shape)
        else:
            a = np.ascontiguousarray(np.asarray(a).astype(np.complex64))
            tau = np.array(tau, dtype=np.float32)
            if a.ndim == 4 and tau.ndim == 2 and tau.shape == (a.shape[0], a.shape[2]):
                pad = ~np.any(a != 0, axis=(1, 3))                         # [E, L]
                tau[pad & ~(np.isfinite(tau) & (tau >= 0))] = 0.0
            self.a, self.tau = a, np.ascontiguousarray(tau)
            shape_a, shape_t = a.shape, tau.shape
        if len(shape_a) != 4 or len(shape_t) != 2 or shape_t != (shape_a[0], shape_a[2]):
            raise ValueError(f"a must be [E, A, L, Ta] and tau [E, L], got {shape_a} and {shape_t}")
        E, _, L, Ta = shape_a
        if not 1 <= E <= MAX_EXAMPLES or not 1 <= L <= MAX_PATHS or Ta not in (1, NUM_SYMBOLS):
            raise ValueError(f"need 1..2^24 examples, 1..1024 paths and 1 or 14 time steps, got {shape_a}")
        if not _is_tensor(a) and not (np.isfinite(self.tau).all() and (self.tau >= 0).all()
                                      and np.isfinite(self.a.view(np.float32)).all()):
            raise ValueError("a and tau must be finite, tau >= 0 (on every path with a non-zero coefficient)")

    num_examples = property(lambda self: int(self.a.shape[0]))
    num_rx_ant = property(lambda self: int(self.a.shape[1]))
    num_paths = property(lambda self: int(self.a.shape[2]))
    num_time_steps = property(lambda self: int(self.a.shape[3]))

    @classmethod
    def from_sionna(cls, a, tau) -> "CIRDataset":
        """the reference's layout: ``a [N, 1, A, 1, 1, L, Ta]`` (one receiver, one single-antenna transmitter)
        and ``tau [N, 1, 1, L]``"""
        a, tau = np.asarray(a), np.asarray(tau)
        if a.ndim != 7 or a.shape[1] != 1 or a.shape[3] != 1 or a.shape[4] != 1:
            raise ValueError(f"a must be [N, 1, A, 1, 1, L, Ta], got {a.shape}")
        if tau.ndim != 4 or tau.shape[1] != 1 or tau.shape[2] != 1:
            raise ValueError(f"tau must be [N, 1, 1, L], got {tau.shape}")
        return cls(a[:, 0, :, 0, 0], tau[:, 0, 0])

    def numpy(self) -> "CIRDataset":
        if not _is_tensor(self.a):
            return self
        return CIRDataset(self.a.cpu().numpy(), self.tau.cpu().numpy())

    def save(self, path: str) -> None:
        d = self.numpy()
        with open(path, "wb") as f:             # a file object: np.savez would append ".npz" to a bare name
            np.savez(f, a=d.a, tau=d.tau)

    @classmethod
    def load(cls, path: str) -> "CIRDataset":
        with np.load(path) as z:
            if set(z.files) != {"a", "tau"}:
                raise ValueError(f"{path}: a CIR dataset holds exactly the keys 'a' and 'tau', got {sorted(z.files)}")
            return cls(z["a"], z["tau"])

    def to(self, device) -> "CIRDataset":
        import torch
        if _is_tensor(self.a):
            return CIRDataset(self.a.to(device), self.tau.to(device))
        return CIRDataset(torch.from_numpy(self.a).to(device), torch.from_numpy(self.tau).to(device))


@dataclasses.dataclass
class CIRChannel:
    """How a ``SlotGenerator`` replays a dataset (include/nrx.h nrx_gen_cir).  ``select``: ``"random"`` (any
    example per (slot, user)), ``"trajectory"`` (user u on the examples that are u modulo U, the reference's
    evaluation rule) or ``"index"`` (the caller passes ``cir_index [B, U]`` int32 with every call).
    ``f_offset``: ``"centered"`` (-F / 2, Sionna's ``subcarrier_frequencies``), ``"zero"`` (the built-in
    generator's) or a number of subcarriers."""
    dataset: CIRDataset
    select: str = "random"
    normalize: bool = True
    f_offset: object = "centered"

    def __post_init__(self):
        if self.select not in SELECT:
            raise ValueError(f"select must be one of {tuple(SELECT)}, got {self.select!r}")
        if isinstance(self.f_offset, str) and self.f_offset not in ("centered", "zero"):
            raise ValueError(f"f_offset must be 'centered', 'zero' or a number, got {self.f_offset!r}")

    def offset(self, num_subcarriers: int) -> float:
        if self.f_offset == "centered":
            return -float(num_subcarriers // 2)
        return 0.0 if self.f_offset == "zero" else float(self.f_offset)


def one_path(num_rx_ant: int, num_examples: int = 1) -> CIRDataset:
    """flat unit channels: one static path of delay 0 per example, example e arriving on the DFT beam
    ``exp(2 pi j e k / A)`` over the antennas k -- orthogonal between examples that differ modulo A, so users on
    different examples (``select="trajectory"``) can be told apart"""
    k, e = np.arange(num_rx_ant)[None, :], np.arange(num_examples)[:, None]
    a = np.exp(2j * np.pi * e * k / num_rx_ant).astype(np.complex64)
    return CIRDataset(a[:, :, None, None], np.zeros((num_examples, 1), np.float32))
