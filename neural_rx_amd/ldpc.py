"""Quasi-cyclic LDPC codes, the GPU decoder and the coded error counters of an evaluation.

A QC-LDPC code is data -- a base matrix of circulant shifts -- and the decoder (``nrx_ldpc_decode``,
include/nrx.h, where the schedule is defined) takes that table as an argument.  The project ships
and tests only codes it constructs itself (``make_regular_qc``: regular, free of 4-cycles); the TS
38.212 base graphs are neither shipped nor reconstructed.  A caller who owns them passes them as a
``QCCode`` through the same path, untested against 38.212.

The evaluation needs no encoder: the generator sends i.i.d. uniform bits ``c``, which are read as
the all-zero codeword under the random scrambler ``c``.  The descrambled LLR ``(2c - 1) L`` is
decoded towards the all-zero word by a sign-symmetric decoder, which has the block-error statistics
of sending random codewords of the coset ``code + c`` (the i.i.d. channel adapter of Hou, Siegel and
Milstein); it holds for any detector that does not exploit the code, and every system here is one.
Stated departures from the reference's ``TBDecoder``: the project's own codes; no CRC, no
segmentation and no bit interleaver; a layered schedule where Sionna's is flooding.  ``no`` is the
one of ``ebno_to_no`` and is not re-adjusted by the code's rate, so absolute Eb/N0 is not comparable
with the reference's tables; the gaps between systems are.
"""
from __future__ import annotations

import ctypes
import dataclasses
import json
import os
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._call import Workspace, fill_grid, fill_mcs, ptr, ref, stream_of, torch as _torch

MAX_Z = 384
CN_TYPES = {"boxplus": 0, "minsum": 1}
# name: (column weight, row weight, base columns); rate (nb - mb) / nb
NAMED = {"r12": (3, 6, 24), "r23": (3, 9, 36), "r34": (3, 12, 24), "r13": (4, 6, 24)}
SEED = 2024
TABLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ldpc_tables.json")


@dataclasses.dataclass
class QCCode:
    """``shifts`` int16 [mb][nb]: -1 no edge, else 0..z-1; block (i, j) with shift s connects check
    ``i z + r`` to variable ``j z + (r + s) mod z``.  Errors are counted over the columns ``< kb z``."""
    mb: int
    nb: int
    z: int
    kb: int
    shifts: np.ndarray
    name: str = ""

    def __post_init__(self):
        self.shifts = np.ascontiguousarray(self.shifts, np.int16).reshape(self.mb, self.nb)

    @property
    def n(self) -> int:
        return self.nb * self.z

    @property
    def num_info(self) -> int:
        return self.kb * self.z

    @property
    def rate(self) -> float:
        return self.kb / self.nb


def has_4cycle(shifts: np.ndarray, z: int) -> bool:
    """columns j != j' sharing rows i != i' with (s[i][j] - s[i'][j] - s[i][j'] + s[i'][j']) mod z == 0"""
    s = np.asarray(shifts, np.int64)
    mb, nb = s.shape
    for i in range(mb):
        for k in range(i + 1, mb):
            both = np.nonzero((s[i] >= 0) & (s[k] >= 0))[0]
            d = (s[i, both] - s[k, both]) % z
            if len(np.unique(d)) != len(d):
                return True
    return False


def make_regular_qc(dv: int, dc: int, nb: int, z: int, seed: int, name: str = "") -> QCCode:
    """A regular QC code: column weight dv, row weight dc (mb = nb dv / dc), the dv rows of a column
    distinct, every shift redrawn until it closes no 4-cycle; kb = nb - mb.  Draws come from
    ``numpy.random.RandomState(seed)``, whose stream numpy keeps frozen."""
    if (nb * dv) % dc or not 2 <= z <= MAX_Z:
        raise ValueError(f"nb dv must be a multiple of dc and z in 2..{MAX_Z}")
    mb = nb * dv // dc
    if not dv <= mb < nb:
        raise ValueError(f"need dv <= mb < nb, got mb = {mb}")
    rng = np.random.RandomState(seed)
    shifts = np.full((mb, nb), -1, np.int64)
    cap = np.full(mb, dc)
    for j in range(nb):
        # the dv rows with the most room, ties in random order: the row weights stay within one of
        # each other, so every row ends at exactly dc
        order = rng.permutation(mb)
        rows = np.sort(order[np.argsort(-cap[order], kind="stable")[:dv]])
        cap[rows] -= 1
        placed = []
        for i in rows:
            for _ in range(100 * z):
                s = int(rng.randint(z))
                good = True
                for k in placed:
                    both = np.nonzero((shifts[i, :j] >= 0) & (shifts[k, :j] >= 0))[0]
                    if np.any((s - shifts[k, j] - shifts[i, both] + shifts[k, both]) % z == 0):
                        good = False
                        break
                if good:
                    break
            else:
                raise ValueError(f"no 4-cycle-free shift for block ({i}, {j}) at z = {z}")
            shifts[i, j] = s
            placed.append(i)
    return QCCode(mb, nb, z, nb - mb, shifts.astype(np.int16), name)


_tables = None


def _committed():
    global _tables
    if _tables is None:
        with open(TABLES, encoding="utf-8") as f:
            _tables = json.load(f)
    return _tables


def named_code(name: str, z: int) -> QCCode:
    """The code ``name`` of ``NAMED`` at lifting size z: the committed table (ldpc_tables.json) where
    there is one -- so that results do not hang on a generator version -- else constructed."""
    if name not in NAMED:
        raise ValueError(f"unknown code {name!r}: one of {sorted(NAMED)}")
    dv, dc, nb = NAMED[name]
    t = _committed().get(f"{name}_z{z}")
    if t is not None:
        return QCCode(t["mb"], t["nb"], t["z"], t["kb"], np.asarray(t["shifts"], np.int16), name)
    return make_regular_qc(dv, dc, nb, z, SEED, name)


def fit(code_name: str, coded_bits: int):
    """(code, C): C = ceil(E / (nb 384)) codewords per (slot, user) and z = floor(E / (C nb)); the
    E - C nb z left-over bits are not used."""
    nb = NAMED[code_name][2]
    C = -(-int(coded_bits) // (nb * MAX_Z))
    z = int(coded_bits) // (C * nb)
    if z < 2:
        raise ValueError(f"{coded_bits} coded bits are too few for {code_name} (nb = {nb})")
    return named_code(code_name, z), C


@dataclasses.dataclass
class DecoderSpec:
    """what ``sim_ber(coded=...)`` decodes with"""
    code_name: str = "r12"
    num_iter: int = 20
    cn_type: str = "boxplus"
    ms_scale: float = 0.75
    llr_clip: float = 20.0
    early_stop: bool = True


class Decoder:
    """``nrx_ldpc_create`` / ``nrx_ldpc_workspace_size`` / ``nrx_ldpc_decode`` for one code on one device."""

    def __init__(self, code: QCCode, device: int = 0):
        self.code, self.device = code, device
        self._lib = _lib.load()
        c = _lib.nrx_ldpc_code()
        c.mb, c.nb, c.z, c.kb = code.mb, code.nb, code.z, code.kb
        c.shifts = code.shifts.ctypes.data
        h = ctypes.c_void_p()
        _lib.check(self._lib.nrx_ldpc_create(ctypes.byref(c), device, ctypes.byref(h)))
        self._h = h
        self._ws = Workspace()
        self.last_workspace_bytes = 0

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.nrx_ldpc_destroy(self._h)
            self._h = None

    def decode(self, llr_in, num_iter: int = 20, cn_type="boxplus", ms_scale: float = 0.75, early_stop: bool = True,
               llr_clip: float = 20.0, skip=None, want_app: bool = False, out=None, stream=None):
        """llr_in [num_cw, N] f32 (log p(0)/p(1)) on the device, skip [num_cw] u8 or None ->
        dict(hard u8 [num_cw, N], app f32 or None, iters i32 [num_cw], parity_ok u8 [num_cw]).
        Asynchronous on the stream; ``out``: a dict of a previous call to write into."""
        torch = _torch()
        N = self.code.n
        if llr_in.dtype != torch.float32 or llr_in.dim() != 2 or llr_in.shape[1] != N or not llr_in.is_contiguous():
            raise ValueError(f"llr_in must be a contiguous float32 [num_cw, {N}] tensor")
        n, dev = llr_in.shape[0], llr_in.device
        if skip is not None and (skip.dtype != torch.uint8 or tuple(skip.shape) != (n,) or skip.device != dev):
            raise ValueError(f"skip must be uint8 [{n}] on {dev}")
        if out is None or out["hard"].shape[0] != n or (want_app and out["app"] is None):
            out = dict(hard=torch.empty((n, N), dtype=torch.uint8, device=dev),
                       app=torch.empty((n, N), dtype=torch.float32, device=dev) if want_app else None,
                       iters=torch.empty(n, dtype=torch.int32, device=dev),
                       parity_ok=torch.empty(n, dtype=torch.uint8, device=dev))
        io = _lib.nrx_ldpc_io()
        io.num_cw, io.num_iter, io.early_stop = n, int(num_iter), int(bool(early_stop))
        io.cn_type = CN_TYPES[cn_type] if isinstance(cn_type, str) else int(cn_type)
        io.ms_scale, io.llr_clip = float(ms_scale), float(llr_clip)
        io.llr_in, io.skip = ptr(llr_in), ptr(skip)
        io.hard, io.iters, io.parity_ok = ptr(out["hard"]), ptr(out["iters"]), ptr(out["parity_ok"])
        io.app = ptr(out["app"]) if want_app else None
        self.last_workspace_bytes = self._ws.size(self._lib.nrx_ldpc_workspace_size, self._h, ref(io))
        ws = self._ws.get(self.last_workspace_bytes, dev)
        _lib.check(self._lib.nrx_ldpc_decode(self._h, ref(io), ws.data_ptr(), ws.numel(), stream_of(dev, stream)))
        return out


def gather(llr, bits, active, mcs, mcs_bits: Sequence[int], dmrs_symbols: Sequence[int], C: int, n_tx: int, N: int,
           tx_col=None, col_prior=None, out=None, stream=None):
    """``nrx_ldpc_gather``: llr [H, B, U, F, T, stride] f32 (Sionna sign), bits [B, U, F, T, stride] u8,
    active [B, U] f32, mcs [B, U] u8 or None -> (llr_in [B U C, N] f32, skip [B U C] u8)."""
    torch = _torch()
    lib = _lib.load()
    H, B, U, F, T, bs = llr.shape
    dev = llr.device
    for name, t in dict(llr=llr, bits=bits, active=active, mcs=mcs, tx_col=tx_col, col_prior=col_prior).items():
        if t is not None and (t.device != dev or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous tensor on {dev}")
    if tuple(bits.shape) != (B, U, F, T, bs) or bits.dtype != torch.uint8 or llr.dtype != torch.float32:
        raise ValueError(f"llr must be float32 and bits uint8 {(B, U, F, T, bs)}")
    if tuple(active.shape) != (B, U) or active.dtype != torch.float32:
        raise ValueError(f"active must be float32 {(B, U)}")
    if mcs is not None and (tuple(mcs.shape) != (B, U) or mcs.dtype != torch.uint8):
        raise ValueError(f"mcs must be uint8 {(B, U)}")
    if tx_col is not None and (tx_col.dtype != torch.int32 or tuple(tx_col.shape) != (n_tx,)):
        raise ValueError(f"tx_col must be int32 [{n_tx}]")
    if col_prior is not None and (col_prior.dtype != torch.float32 or tuple(col_prior.shape) != (N,)):
        raise ValueError(f"col_prior must be float32 [{N}]")
    if out is None:
        out = (torch.empty((B * U * C, N), dtype=torch.float32, device=dev),
               torch.empty(B * U * C, dtype=torch.uint8, device=dev))
    io = _lib.nrx_ldpc_gather_io()
    fill_grid(io, B, U, F, T)
    fill_mcs(io, mcs_bits, dmrs_symbols, bits_stride=bs, num_heads=H)
    io.num_cw_per_user, io.n_tx, io.n = int(C), int(n_tx), int(N)
    io.llr, io.bits, io.active, io.mcs = ptr(llr), ptr(bits), ptr(active), ptr(mcs)
    io.tx_col, io.col_prior = ptr(tx_col), ptr(col_prior)
    io.llr_in, io.skip = ptr(out[0]), ptr(out[1])
    _lib.check(lib.nrx_ldpc_gather(ref(io), stream_of(dev, stream)))
    return out


def count(hard, skip, B: int, U: int, C: int, num_info: int, counts, iters=None, iter_counts=None, stream=None):
    """``nrx_ldpc_count``: counts [U, 4] i64 += (information-bit errors, information bits, block errors,
    blocks); iter_counts [U, 2] i64 += (decoder iterations, codewords)."""
    torch = _torch()
    lib = _lib.load()
    io = _lib.nrx_ldpc_count_io()
    io.batch, io.num_tx, io.num_cw_per_user, io.n, io.num_info = B, U, C, hard.shape[1], int(num_info)
    if tuple(hard.shape) != (B * U * C, hard.shape[1]) or hard.dtype != torch.uint8 or not hard.is_contiguous():
        raise ValueError(f"hard must be a contiguous uint8 [{B * U * C}, N] tensor")
    if tuple(skip.shape) != (B * U * C,) or skip.dtype != torch.uint8:
        raise ValueError(f"skip must be uint8 [{B * U * C}]")
    if tuple(counts.shape) != (U, 4) or counts.dtype != torch.int64 or not counts.is_contiguous():
        raise ValueError(f"counts must be a contiguous int64 [{U}, 4] tensor")
    io.hard, io.skip, io.counts = hard.data_ptr(), skip.data_ptr(), counts.data_ptr()
    if iters is not None and iter_counts is not None:
        if iters.dtype != torch.int32 or tuple(iter_counts.shape) != (U, 2) or iter_counts.dtype != torch.int64:
            raise ValueError(f"iters must be int32 and iter_counts int64 [{U}, 2]")
        io.iters, io.iter_counts = iters.data_ptr(), iter_counts.data_ptr()
    _lib.check(lib.nrx_ldpc_count(ref(io), stream_of(hard, stream)))
    return counts


@dataclasses.dataclass
class CodedResult:
    """Coded figures of one Eb/N0 point.  ``no`` of the point is the one of ``ebno_to_no``: it is not
    re-adjusted by the code's rate."""
    ber: float                        # information-bit errors / information bits
    bler: float                       # (slot, user) blocks with an information-bit error / blocks
    mean_iters: float                 # decoder iterations per codeword
    counts: list                      # [information-bit errors, information bits, block errors, blocks]
    codewords: int
    code: str
    rate: float                       # kb / nb
    n: int                            # N
    z: int
    cw_per_block: int                 # C
    num_iter: int
    cn_type: str
    ebno_rate_adjusted: bool = False

    def as_dict(self):
        return dataclasses.asdict(self)


class CodedAccumulator:
    """Gather, decode and count of every batch of one Eb/N0 point, modelled on
    ``softmetrics.SoftAccumulator``: ``add`` is asynchronous on the stream, ``reduce`` sums over the
    ranks of a process group, ``result`` copies to the host.  The int64 accumulators are views of one
    tensor ``i64`` ([U, 4] counters in the layout of ``nrx_count_errors``, then [U, 2] iteration
    counters), so that a reduction is one collective."""

    def __init__(self, spec: DecoderSpec, num_tx: int, mcs_bits: Sequence[int], num_data_re: int, device: int = 0):
        torch = _torch()
        self.spec, self.num_tx, self.mcs_bits = spec, int(num_tx), [int(b) for b in mcs_bits]
        if spec.cn_type not in CN_TYPES:
            raise ValueError(f"cn_type must be one of {sorted(CN_TYPES)}")
        # sized by the widest MCS; a user of a narrower one has fewer codewords, the rest are skipped
        self.code, self.C = fit(spec.code_name, num_data_re * max(self.mcs_bits))
        self.n_tx = self.code.n
        self.decoder = Decoder(self.code, device)
        self.device = device
        U = self.num_tx
        self.i64 = torch.zeros(U * 6, dtype=torch.int64, device=f"cuda:{device}")
        self.counts = self.i64[:U * 4].view(U, 4)
        self.iter_counts = self.i64[U * 4:].view(U, 2)
        self._gathered = None
        self._decoded = None
        self._total = None
        self.last = None              # (llr_in, skip, decoder outputs) of the last add

    def reset(self):
        self.i64.zero_()
        self._total = None

    def add(self, llr, bits, active, mcs, dmrs_symbols: Sequence[int], stream=None):
        s = self.spec
        B, U = llr.shape[1], llr.shape[2]
        if U != self.num_tx:
            raise ValueError(f"llr has {U} users, the accumulator {self.num_tx}")
        if self._gathered is not None and self._gathered[0].shape[0] != B * U * self.C:
            self._gathered = self._decoded = None
        self._gathered = gather(llr, bits, active, mcs, self.mcs_bits, dmrs_symbols, self.C, self.n_tx, self.code.n,
                                out=self._gathered, stream=stream)
        llr_in, skip = self._gathered
        self._decoded = self.decoder.decode(llr_in, s.num_iter, s.cn_type, s.ms_scale, s.early_stop, s.llr_clip,
                                            skip=skip, out=self._decoded, stream=stream)
        count(self._decoded["hard"], skip, B, U, self.C, self.code.num_info, self.counts, self._decoded["iters"],
              self.iter_counts, stream=stream)
        self.last = (llr_in, skip, self._decoded)
        self._total = None

    def reduce(self, dist=None):
        i64 = self.i64.clone()
        if dist is not None:
            if dist.get_backend() != "nccl":
                i64 = i64.cpu()
            dist.all_reduce(i64)
        self._total = i64.cpu()
        return self

    def result(self) -> CodedResult:
        i64 = (self._total if self._total is not None else self.i64.cpu()).numpy()
        U = self.num_tx
        c = i64[:U * 4].reshape(U, 4).sum(0)
        it = i64[U * 4:].reshape(U, 2).sum(0)
        nan = float("nan")
        return CodedResult(ber=float(c[0] / c[1]) if c[1] else nan, bler=float(c[2] / c[3]) if c[3] else nan,
                           mean_iters=float(it[0] / it[1]) if it[1] else nan, counts=[int(v) for v in c],
                           codewords=int(it[1]), code=self.spec.code_name, rate=self.code.rate, n=self.code.n,
                           z=self.code.z, cw_per_block=self.C, num_iter=self.spec.num_iter, cn_type=self.spec.cn_type)


def write_tables(path: str = TABLES, sizes=(("r12", 96), ("r23", 64), ("r34", 96), ("r13", 96))):
    """Regenerate the committed tables (tests/test_ldpc_ref.py checks that they regenerate identically)."""
    d = {}
    for name, z in sizes:
        dv, dc, nb = NAMED[name]
        c = make_regular_qc(dv, dc, nb, z, SEED, name)
        d[f"{name}_z{z}"] = dict(mb=c.mb, nb=c.nb, z=c.z, kb=c.kb, seed=SEED, shifts=c.shifts.tolist())
    with open(path, "w", encoding="utf-8") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v)}' for k, v in d.items()) + "\n}\n")


if __name__ == "__main__":
    write_tables()
