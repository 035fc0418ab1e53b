"""Training of the CGNN on the GPU: loss, gradient and Adam in ``libnrx.so`` (include/nrx.h ``nrx_train_grad`` /
``nrx_train_grad_acc`` / ``nrx_adam_step``), slots from ``generator.SlotGenerator``.

The counterpart of the reference's training loop (``scripts/train_neural_rx.py``, ``utils/utils.py:148-428``; loss
at ``utils/neural_rx.py:860-879``): binary cross-entropy on the LLRs plus ``w_chest`` times the mean squared error
of the channel readout, under Keras Adam.

    python -m neural_rx_amd.train -config_name nrx_rt -num_prbs 4 -steps 200 -batch_size 128 \
        -ebno_db_min 0 -ebno_db_max 12 -init shipped -out tuned.npz
    python -m neural_rx_amd.train -config_name nrx_rt -num_prbs 4 -schedule tests/golden/config/nrx_rt.cfg \
        -schedule_scale 1e-4 -micro_batch 32 -per_slot_ebno -save_every 50 -out tuned.npz [-num_gpus 8]
    python -m neural_rx_amd.train ... -resume tuned.npz.state.npz
    python -m neural_rx_amd.evaluate -config_name nrx_rt -num_prbs 4 -weights tuned.npz

One Adam step is built from micro-batches (``Trainer.grad_micro``: the first call overwrites the gradient, the
others accumulate, every loss denominator carries the step's whole batch) and, with ``-num_gpus``, from ranks
(``Trainer.all_reduce``: one sum of the flat gradient).  Step k of a global batch Bg uses the global slots
``[k Bg, (k + 1) Bg)``; rank r takes its ``parallel.shard_range`` of them.  Every random choice of step k is a
function of ``(seed, k)`` and of global slot indices, never of the draws before, the rank or the split, so the
step's gradient is the same function whatever the world size and the micro-batch size (up to the float32
summation order) and a run resumed from a checkpoint repeats the uninterrupted run bit for bit.

With ``-schedule`` (a reference-format cfg, ``config.parse_schedule``) or ``-per_slot_ebno`` the sampling is the
reference's: the number of active users of a step is ``floor(a + sqrt(u) (b + 1 - a))`` (``utils/utils.py:72-127``,
``222-224``) and every slot draws its own Eb/N0, uniform in the range the schedule gives for that number
(``utils/utils.py:288-290``).  Without them one Eb/N0 is drawn per step and the number of active users uniformly
in 1..``-num_tx_eval``, as before.  What still departs from the reference: the MCS-dependent SNR offsets and MCS
sampling probabilities, trainable transmitters, and the channel (the generator's, not UMi).
"""
from __future__ import annotations

import argparse
import ctypes
import os
from typing import List, Sequence

import numpy as np

from . import _lib
from ._call import Workspace, ptr, require, stream_of, torch as _torch
from .config import ModelSpec

NUM_SYMBOLS = 14


class Trainer:
    """Flat ``w``, ``g``, ``m``, ``v`` device tensors of one topology (the arrays of ``nrx_weight_layout``
    concatenated in Keras ``get_weights()`` order) and the workspace of ``nrx_train_grad``."""

    def __init__(self, spec: ModelSpec, weight_list: Sequence[np.ndarray], device: int = 0):
        torch = _torch()
        self.spec = spec
        self.device = device
        self._lib = _lib.load()
        self._desc = _lib.make_desc(spec)
        n = ctypes.c_int32()
        _lib.check(self._lib.nrx_weight_layout(ctypes.byref(self._desc), ctypes.byref(n), None, 0))
        sizes = (ctypes.c_int64 * n.value)()
        _lib.check(self._lib.nrx_weight_layout(ctypes.byref(self._desc), ctypes.byref(n), sizes, n.value))
        if len(weight_list) != n.value:
            raise ValueError(f"expected {n.value} weight arrays, got {len(weight_list)}")
        arrs = [np.ascontiguousarray(w, dtype=np.float32) for w in weight_list]
        for i, (a, s) in enumerate(zip(arrs, sizes)):
            if a.size != s:
                raise ValueError(f"weight {i}: {a.shape} has {a.size} elements, expected {s}")
        self._shapes = [a.shape for a in arrs]
        self._dev = torch.device("cuda", device)
        self.w = torch.from_numpy(np.concatenate([a.ravel() for a in arrs])).to(self._dev)
        self.g = torch.zeros_like(self.w)
        self.m = torch.zeros_like(self.w)
        self.v = torch.zeros_like(self.w)
        self.loss = torch.zeros(2, dtype=torch.float64, device=self._dev)
        self.num_steps = 0
        self._ws = Workspace()

    def _io(self, sb, pe, num_it, multiloss, w_chest, dmrs_symbols, llr=None, h_ref=None):
        torch = _torch()
        sp = self.spec
        B, U, F = sb.bits.shape[0], sb.bits.shape[1], sb.bits.shape[2]
        A2 = 2 * sp.num_rx_ant
        f32 = torch.float32
        require("y", sb.y, (B, F, NUM_SYMBOLS, A2), f32, self._dev)
        require("pe", pe, (U, F, NUM_SYMBOLS, 2), f32, self._dev)
        require("active", sb.active, (B, U), f32, self._dev)
        require("bits", sb.bits, None, torch.uint8, self._dev)
        for name, t in (("h_hat", sb.h_hat if sp.use_h_hat else None), ("h", sb.h)):
            if t is not None:
                require(name, t, (B, U, F, NUM_SYMBOLS, A2), f32, self._dev)
        mask = sb.mcs_mask if sp.num_mcs > 1 else None
        if mask is not None:
            require("mcs_mask", mask, (B, U, sp.num_mcs), f32, self._dev)
        io = _lib.nrx_train_io()
        io.shape = _lib.nrx_shape(B, U, F, NUM_SYMBOLS)
        io.num_it = sp.num_it if num_it is None else num_it
        io.multiloss, io.w_chest, io.bits_stride = int(bool(multiloss)), float(w_chest), sb.bits.shape[4]
        for t in dmrs_symbols:
            io.dmrs_symbol_mask |= 1 << t
        io.y, io.pe, io.active, io.bits = ptr(sb.y), ptr(pe), ptr(sb.active), ptr(sb.bits)
        io.h_hat, io.mcs_mask, io.h = ptr(sb.h_hat if sp.use_h_hat else None), ptr(mask), ptr(sb.h)
        io.weights, io.grad, io.loss = ptr(self.w), ptr(self.g), ptr(self.loss)
        io.llr, io.h_ref = ptr(llr), ptr(h_ref)
        return io

    def workspace_bytes(self, io) -> int:
        s = io.shape
        return self._ws.size(self._lib.nrx_train_workspace_size, ctypes.byref(self._desc), ctypes.byref(io),
                             key=(s.batch, s.num_tx, s.num_subcarriers, io.num_it, io.multiloss))

    def grad_async(self, slot_batch, pe, num_it=None, multiloss=False, w_chest=0.0, dmrs_symbols=(2, 11),
                   want_outputs=False, stream=None, workspace=None, accumulate=False, batch_total=None):
        """Launch ``nrx_train_grad`` on the batch (a ``generator.SlotBatch`` with ``h`` when ``w_chest > 0``): the
        gradient of ``loss_data + w_chest loss_chest`` lands in ``self.g``, the two losses in ``self.loss``
        (device, float64).  Nothing synchronises.  ``want_outputs``: also return ``(llr, h_ref)`` of the last
        readout, in the engine's layouts.  ``accumulate`` / ``batch_total``: the batch is a micro-batch of a step
        of ``batch_total`` slots (``nrx_train_grad_acc``): the gradient and the losses are added onto what
        ``self.g`` and ``self.loss`` hold, and the loss denominators carry ``batch_total``."""
        torch = _torch()
        sp = self.spec
        out = (None, None)
        if want_outputs:
            B, U, F = slot_batch.bits.shape[:3]
            out = (torch.empty((sp.num_llr_heads, B, U, F, NUM_SYMBOLS, sp.bits_max), dtype=torch.float32,
                               device=self._dev),
                   torch.empty((B, U, F, NUM_SYMBOLS, 2 * sp.num_rx_ant), dtype=torch.float32, device=self._dev))
        io = self._io(slot_batch, pe, num_it, multiloss, w_chest, dmrs_symbols, *out)
        ws = self._ws.get(self.workspace_bytes(io) if workspace is None else 0, self._dev, workspace)
        if not accumulate and batch_total is None:
            _lib.check(self._lib.nrx_train_grad(ctypes.byref(self._desc), ctypes.byref(io), ws.data_ptr(), ws.numel(),
                                                stream_of(self.w, stream)))
            return out
        acc = _lib.nrx_train_acc(int(bool(accumulate)), io.shape.batch if batch_total is None else int(batch_total))
        _lib.check(self._lib.nrx_train_grad_acc(ctypes.byref(self._desc), ctypes.byref(io), ctypes.byref(acc),
                                                ws.data_ptr(), ws.numel(), stream_of(self.w, stream)))
        return out

    def grad_micro(self, batches, pe, num_it=None, multiloss=False, w_chest=0.0, dmrs_symbols=(2, 11),
                   batch_total=None, accumulate=False, stream=None):
        """One step's gradient from the slot batches ``batches`` (of any sizes): the first call overwrites
        ``self.g`` and ``self.loss`` (with ``accumulate`` it adds too), the others accumulate, and the loss
        denominators carry ``batch_total`` (default: the sum of the batches), so ``self.g`` ends as the gradient
        of the whole batch.  All calls share one workspace, sized for the largest micro-batch.  Nothing
        synchronises."""
        batches = list(batches)
        total = sum(sb.bits.shape[0] for sb in batches) if batch_total is None else int(batch_total)
        ios = [self._io(sb, pe, num_it, multiloss, w_chest, dmrs_symbols) for sb in batches]
        ws = self._ws.get(max([self.workspace_bytes(io) for io in ios], default=0), self._dev)
        for i, sb in enumerate(batches):
            self.grad_async(sb, pe, num_it, multiloss, w_chest, dmrs_symbols, stream=stream, workspace=ws,
                            accumulate=accumulate or i > 0, batch_total=total)

    def all_reduce(self, group=None):
        """Sum ``self.g`` and ``self.loss`` over the process group, in place: one collective for the flat gradient
        and a small one for the two losses.  Over "nccl" (RCCL, one GPU per rank) the device buffers are reduced;
        over gloo (ranks that share a device) they are staged through the host.  Every rank ends with the same
        bits, so every rank takes the same Adam step and the weights never need a broadcast.  With
        ``batch_total`` = the global batch in every rank's gradient calls, the sum is the gradient of the global
        batch: nothing is scaled.  A no-op without an initialised group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        if dist.get_backend(group) == "nccl":
            dist.all_reduce(self.g, op=dist.ReduceOp.SUM, group=group)
            dist.all_reduce(self.loss, op=dist.ReduceOp.SUM, group=group)
            return
        for t in (self.g, self.loss):
            host = t.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
            t.copy_(host)

    def save_state(self, path, global_step=None):
        """Write ``w``, ``m``, ``v``, ``num_steps`` and the loop's global step (default: ``num_steps``) as an
        ``.npz`` that ``weights.load_file`` still reads for the weights alone."""
        arrays = {f"w{i:03d}": a for i, a in enumerate(self.weights())}
        with open(path, "wb") as f:
            np.savez(f, count=np.int64(len(arrays)), adam_m=self.m.cpu().numpy(), adam_v=self.v.cpu().numpy(),
                     num_steps=np.int64(self.num_steps),
                     global_step=np.int64(self.num_steps if global_step is None else global_step), **arrays)

    def load_state(self, path) -> int:
        """Restore what ``save_state`` wrote; returns the global step"""
        torch = _torch()
        with np.load(path, allow_pickle=False) as d:
            if "adam_m" not in d:
                raise ValueError(f"{path} holds weights only, no optimizer state")
            ws = [np.ascontiguousarray(d[f"w{i:03d}"], dtype=np.float32) for i in range(int(d["count"]))]
            if [a.shape for a in ws] != list(self._shapes):
                raise ValueError(f"{path} holds the weights of another topology")
            m, v = d["adam_m"], d["adam_v"]
            if m.shape != (self.w.numel(),) or v.shape != m.shape or m.dtype != np.float32 or v.dtype != np.float32:
                raise ValueError(f"{path}: m and v must be float32 [{self.w.numel()}]")
            self.w.copy_(torch.from_numpy(np.concatenate([a.ravel() for a in ws])))
            self.m.copy_(torch.from_numpy(m))
            self.v.copy_(torch.from_numpy(v))
            self.num_steps = int(d["num_steps"])
            return int(d["global_step"])

    def grad(self, slot_batch, pe, num_it=None, multiloss=False, w_chest=0.0, dmrs_symbols=(2, 11)):
        """``grad_async`` and the losses on the host: ``(loss_data, loss_chest)``"""
        self.grad_async(slot_batch, pe, num_it, multiloss, w_chest, dmrs_symbols)
        ld, lc = self.loss.tolist()
        return ld, lc

    def step(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, stream=None):
        """One Keras-Adam update of ``w`` with the gradient in ``g``"""
        self.num_steps += 1
        io = _lib.nrx_adam_io()
        io.n, io.w, io.g, io.m, io.v = self.w.numel(), ptr(self.w), ptr(self.g), ptr(self.m), ptr(self.v)
        io.lr, io.beta1, io.beta2, io.eps, io.step = lr, beta1, beta2, eps, self.num_steps
        _lib.check(self._lib.nrx_adam_step(ctypes.byref(io), stream_of(self.w, stream)))

    def _split(self, flat) -> List[np.ndarray]:
        a = flat.cpu().numpy()
        out, o = [], 0
        for s in self._shapes:
            n = int(np.prod(s))
            out.append(a[o:o + n].reshape(s).copy())
            o += n
        return out

    def weights(self) -> List[np.ndarray]:
        """the current weights as the Keras-ordered list"""
        return self._split(self.w)

    def gradients(self) -> List[np.ndarray]:
        """the last gradient, split like ``weights()``"""
        return self._split(self.g)

    def engine(self):
        """a ``CGNNEngine`` on the current weights"""
        from .receiver import CGNNEngine
        return CGNNEngine(self.spec, self.weights(), device=self.device)


# ---------------------------------------------------------------- the loop's host side: sampling and slot accounting
# Every draw of step k comes from its own generator keyed by (what is drawn, seed, k): nothing depends on how many
# draws came before, so a resumed run, another world size or another micro-batch size sees the same values.
_DRAW_NUM_TX, _DRAW_EBNO = 1, 2


def _step_rng(what: int, seed: int, step: int):
    return np.random.default_rng([what, int(seed), int(step)])


def num_tx_law(u, min_num_tx: int, max_num_tx: int):
    """The reference's triangular law on the integers ``a..b``: ``floor(a + sqrt(u) (b + 1 - a))`` for ``u``
    uniform on [0, 1) (``TriangularDistributionSampler(a, b + 1)``), which favours the larger numbers: for 1..2 it
    gives 1 with probability 1/4 and 2 with 3/4.  ``u``: a float or an array."""
    a, b = int(min_num_tx), int(max_num_tx)
    n = np.floor(a + np.sqrt(np.asarray(u, np.float64)) * (b + 1 - a)).astype(np.int64)
    return np.minimum(n, b)           # sqrt(u) rounds to 1.0 for the largest u < 1


def sample_num_tx(seed: int, step: int, min_num_tx: int, max_num_tx: int, law: str = "triangular") -> int:
    """the number of active users of step ``step``: ``num_tx_law`` or, with ``law="uniform"``, uniform on a..b"""
    u = _step_rng(_DRAW_NUM_TX, seed, step).random()
    if law == "uniform":
        return int(min(int(min_num_tx + u * (max_num_tx + 1 - min_num_tx)), max_num_tx))
    return int(num_tx_law(u, min_num_tx, max_num_tx))


def step_ebno_db(seed: int, step: int, batch: int, lo_db: float, hi_db: float, per_slot: bool = True) -> np.ndarray:
    """Eb/N0 [dB] of the ``batch`` global slots of step ``step``, float64: uniform in [lo_db, hi_db], one draw per
    slot or (``per_slot=False``) one for the step.  Drawn for the whole global batch; a rank slices it."""
    rng = _step_rng(_DRAW_EBNO, seed, step)
    if per_slot:
        return rng.uniform(lo_db, hi_db, size=batch)
    return np.full(batch, rng.uniform(lo_db, hi_db))


def micro_ranges(step: int, batch: int, world: int = 1, rank: int = 0, micro_batch: int = 0):
    """The micro-batches of rank ``rank`` in step ``step`` as global slot ranges ``[(lo, hi), ...]``: its
    ``parallel.shard_range`` of ``[step batch, (step + 1) batch)`` cut into pieces of at most ``micro_batch``
    slots (0: one piece)."""
    from .parallel import shard_range
    lo, hi = shard_range(batch, world, rank)
    m = micro_batch if micro_batch and micro_batch > 0 else max(hi - lo, 1)
    base = step * batch
    return [(base + s, base + min(s + m, hi)) for s in range(lo, hi, m)]


def ebno_db_to_no(ebno_db, num_dmrs_symbols: int) -> np.ndarray:
    """``generator.ebno_to_no`` on an array, float64"""
    e = np.asarray(ebno_db, np.float64) - 10.0 * np.log10(1.0 - num_dmrs_symbols / NUM_SYMBOLS)
    return 10.0 ** (-e / 10.0)


def _arguments(argv):
    from . import evaluate
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    evaluate.add_arguments(ap, generator_only=True)
    ap.add_argument("-steps", type=int, default=100)
    ap.add_argument("-ebno_db_min", type=float, default=0.0)
    ap.add_argument("-ebno_db_max", type=float, default=12.0)
    ap.add_argument("-init", default="shipped", help="shipped, seeded, or a weight file (.npz)")
    ap.add_argument("-out", default=None, metavar="FILE.npz", help="write the trained weights here (weights.save)")
    ap.add_argument("-learning_rate", type=float, default=1e-3)
    ap.add_argument("-apply_multiloss", action="store_true")
    ap.add_argument("-weighting_double_readout", type=float, default=0.02,
                    help="weight of the channel-readout loss; 0 switches the double readout off")
    ap.add_argument("-eval_every", type=int, default=50, help="steps between BER prints on the held-out batch")
    ap.add_argument("-eval_ebno_db", type=float, default=None, help="Eb/N0 of the held-out batch (default: mid-range)")
    ap.add_argument("-micro_batch", type=int, default=0, metavar="N",
                    help="slots per gradient call; a step accumulates its micro-batches (0: the whole batch)")
    ap.add_argument("-num_gpus", type=int, default=1, metavar="G",
                    help="data-parallel ranks, one fresh process per GPU (at most 16)")
    ap.add_argument("-schedule", default=None, metavar="FILE.cfg",
                    help="a reference-format cfg whose training_schedule replaces -steps, -batch_size, "
                         "-learning_rate, -apply_multiloss, -weighting_double_readout and the Eb/N0 range")
    ap.add_argument("-schedule_scale", type=float, default=1.0, help="multiplies every num_iter of the schedule")
    ap.add_argument("-save_every", type=int, default=0, metavar="K",
                    help="steps between checkpoints (Trainer.save_state) at OUT.state.npz; needs -out")
    ap.add_argument("-resume", default=None, metavar="FILE", help="continue from a checkpoint of -save_every")
    ap.add_argument("-per_slot_ebno", action="store_true",
                    help="the reference's sampling: one Eb/N0 per slot, triangular law for the active users")
    a = ap.parse_args(argv)
    evaluate.check_arguments(ap, a)
    if a.steps < 0 or a.ebno_db_max < a.ebno_db_min:
        ap.error("-steps must be >= 0 and -ebno_db_max >= -ebno_db_min")
    if a.micro_batch < 0 or a.save_every < 0 or not a.schedule_scale > 0:
        ap.error("-micro_batch and -save_every must be >= 0 and -schedule_scale > 0")
    if not 1 <= a.num_gpus <= 16:
        ap.error("-num_gpus must be 1..16")
    if a.save_every and not a.out:
        ap.error("-save_every needs -out: the checkpoint is written next to it")
    return a


def _plain_schedule(a, max_active):
    """the schedule the plain options describe: one stage, one Eb/N0 range for every number of active users"""
    from .config import ScheduleStage, TrainingSchedule
    st = ScheduleStage(num_iter=a.steps, learning_rate=a.learning_rate, batch_size=a.batch_size,
                       min_training_snr_db=(a.ebno_db_min,) * max_active, max_training_snr_db=(a.ebno_db_max,) * max_active,
                       double_readout=a.weighting_double_readout > 0, apply_multiloss=a.apply_multiloss,
                       weighting_double_readout=a.weighting_double_readout)
    return TrainingSchedule(stages=(st,), min_num_tx=1, max_num_tx=max_active)


def train_loop(a, rank: int = 0, world: int = 1, device: int = 0, record=None, log=print):
    """The training loop of one rank (``a``: the parsed options).  ``record(k, trainer, slot_batches)``, when
    given, is called in every step behind the all-reduce and before the Adam update (tests read ``g`` there;
    ``slot_batches`` are this rank's micro-batches when ``a.keep_batches`` is set, else empty).  Returns the
    ``Trainer``."""
    import torch
    from . import weights as W
    from .config import get_config, parse_schedule
    from .generator import SlotGenerator, count_errors, ebno_to_no
    from .receiver import compute_pe, spec_for
    from . import evaluate
    torch.cuda.set_device(device)
    cfg = get_config(a.config_name)
    spec = spec_for(cfg)
    params, u, _ = evaluate.generator_params(a, cfg)
    max_active = params.num_active
    reference_sampling = a.schedule is not None or a.per_slot_ebno
    if a.schedule is not None:
        sched = parse_schedule(a.schedule).scaled(a.schedule_scale)
        if sched.max_num_tx > params.num_tx:
            raise ValueError(f"the schedule trains up to {sched.max_num_tx} users, the generator has {params.num_tx}")
    else:
        sched = _plain_schedule(a, max_active)
    # the draws of a run without any of the new options are those of the loop before them: one generator, in order
    legacy = not reference_sampling
    init = W.load(cfg.label) if a.init == "shipped" else W.seeded(spec, a.seed) if a.init == "seeded" \
        else W.load_file(a.init)
    tr = Trainer(spec, init, device=device)
    gen = SlotGenerator(params, device=device, want_h=True)
    held = SlotGenerator(params, device=device, want_h=True)       # its own buffers: the batch stays
    dev = torch.device("cuda", device)
    pe = torch.from_numpy(compute_pe(params.num_tx, params.num_subcarriers, params.dmrs_symbols,
                                     params.cdm_group)).to(dev)
    nd = len(params.dmrs_symbols)
    s0 = sched.stages[0]
    eval_ebno = a.eval_ebno_db if a.eval_ebno_db is not None else \
        0.5 * (a.ebno_db_min + a.ebno_db_max) if a.schedule is None else \
        0.5 * (s0.min_training_snr_db[-1] + s0.max_training_snr_db[-1])
    held_sb = held(a.batch_size, ebno_to_no(eval_ebno, nd), slot_offset=1 << 41)    # beyond every training slot

    def held_out_ber():
        eng = tr.engine()
        mask = held_sb.mcs_mask if spec.num_mcs > 1 else None
        llr, _ = eng.forward(held_sb.y, pe, held_sb.h_hat, held_sb.active, mcs_mask=mask,
                             num_it=cfg.num_nrx_iter_eval, want_h=False)
        c = count_errors(llr, held_sb.bits, held_sb.active, held_sb.mcs, params.mcs_bits,
                         params.dmrs_symbols).sum(0).tolist()
        eng.close()
        return c[0] / max(c[1], 1)

    def say(msg):
        if rank == 0:
            log(msg, flush=True)

    start = tr.load_state(a.resume) if a.resume else 0
    total = sched.total_steps
    rng = np.random.default_rng(a.seed)
    if legacy:
        for _ in range(start):          # the draws of the steps already taken, in their order
            rng.uniform(a.ebno_db_min, a.ebno_db_max)
            rng.integers(1, max_active + 1)
    say(f"step {start}  held-out BER {held_out_ber():.4e} at {eval_ebno:g} dB")
    state_path = f"{a.out}.state.npz" if a.out else None
    keep = bool(getattr(a, "keep_batches", False))
    for k in range(start, total):
        si, st = sched.stage_of(k)
        Bg = st.batch_size
        if legacy:
            ebno = np.full(Bg, rng.uniform(a.ebno_db_min, a.ebno_db_max))
            n = int(rng.integers(1, max_active + 1))
        else:
            n = sample_num_tx(a.seed, k, sched.min_num_tx, sched.max_num_tx)
            ebno = step_ebno_db(a.seed, k, Bg, st.min_training_snr_db[n - sched.min_num_tx],
                                st.max_training_snr_db[n - sched.min_num_tx])
        params.num_active = n
        no = ebno_db_to_no(ebno, nd)
        no_dev = torch.from_numpy(no).to(dev) if not legacy else None
        pieces = micro_ranges(k, Bg, world, rank, a.micro_batch)
        kw = dict(multiloss=st.apply_multiloss, w_chest=st.w_chest, dmrs_symbols=params.dmrs_symbols)
        kept = []
        for i, (lo, hi) in enumerate(pieces):
            if legacy:
                sb = gen(hi - lo, ebno_to_no(float(ebno[0]), nd), slot_offset=lo)
            else:
                sb = gen(hi - lo, no_dev[lo - k * Bg:hi - k * Bg], slot_offset=lo)
            if len(pieces) == 1 and world == 1:
                tr.grad_async(sb, pe, **kw)                    # the whole batch in one call: nrx_train_grad
            else:
                tr.grad_async(sb, pe, accumulate=i > 0, batch_total=Bg, **kw)
            if keep:
                kept.append(type(sb)(**{f: (None if v is None else v.clone()) for f, v in vars(sb).items()}))
        if not pieces:                                          # more ranks than slots: this rank adds nothing
            tr.g.zero_()
            tr.loss.zero_()
        tr.all_reduce()
        if record is not None:
            record(k, tr, kept)
        tr.step(lr=st.learning_rate)
        done = k + 1
        if done % a.eval_every == 0 or done == total:
            ld, lc = tr.loss.tolist()
            say(f"step {done}  stage {si}  loss_data {ld:.5f}  loss_chest {lc:.5f}  held-out BER {held_out_ber():.4e}"
                if len(sched.stages) > 1 else
                f"step {done}  loss_data {ld:.5f}  loss_chest {lc:.5f}  held-out BER {held_out_ber():.4e}")
        if a.save_every and rank == 0 and (done % a.save_every == 0 or done == total):
            tr.save_state(state_path + ".tmp", global_step=done)
            os.replace(state_path + ".tmp", state_path)
    if a.out and rank == 0:
        W.save(a.out, tr.weights())
    return tr


def _rank_main(rank, world, port, argv):
    """one data-parallel rank, in a fresh interpreter: its own GPU, RCCL for the gradient"""
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch
    import torch.distributed as dist
    threads = int(os.environ.get("OMP_NUM_THREADS", "4"))       # the environment's budget, shared by the ranks
    torch.set_num_threads(max(1, threads // world))
    a = _arguments(argv)
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    try:
        train_loop(a, rank, world, device=rank)
    finally:
        dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(argv, world):
    """Start ``world`` ranks as fresh interpreters (spawn) and wait for them.  This process never initialises the
    GPU; a rank that fails ends the others."""
    import multiprocessing as mp
    import time
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, list(argv))) for r in range(world)]
    for p in procs:
        p.start()
    failed = None
    while failed is None and any(p.is_alive() for p in procs):
        time.sleep(0.2)
        failed = next((p for p in procs if p.exitcode not in (None, 0)), None)
    for p in procs:
        if failed is not None and p.is_alive():
            p.terminate()
        p.join()
    bad = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode != 0]
    if bad:
        raise SystemExit(f"training rank(s) failed: {bad}")


def main(argv=None):
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    a = _arguments(argv)
    if a.num_gpus > 1:
        if a.gpu is not None:
            raise SystemExit("-gpu and -num_gpus: the ranks take the GPUs 0..G-1")
        _spawn(argv, a.num_gpus)
        return None
    return train_loop(a, device=a.gpu if a.gpu is not None else 0)


if __name__ == "__main__":
    main()
