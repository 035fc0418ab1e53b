"""Training of the CGNN on the GPU: loss, gradient and Adam in ``libnrx.so`` (include/nrx.h ``nrx_train_grad`` /
``nrx_adam_step``), slots from ``generator.SlotGenerator``.

The counterpart of the reference's training loop (``scripts/train_neural_rx.py``, ``utils/utils.py:148-428``; loss
at ``utils/neural_rx.py:860-879``): binary cross-entropy on the LLRs plus ``w_chest`` times the mean squared error
of the channel readout, under Keras Adam.

    python -m neural_rx_amd.train -config_name nrx_rt -num_prbs 4 -steps 200 -batch_size 128 \
        -ebno_db_min 0 -ebno_db_max 12 -init shipped -out tuned.npz
    python -m neural_rx_amd.evaluate -config_name nrx_rt -num_prbs 4 -weights tuned.npz

Two stated departures from the reference's loop: one Eb/N0 is drawn per step, not per slot (the generator takes one
``no`` per call), and the number of active users of a step is drawn uniformly in 1..``-num_tx_eval``.  The
schedule fields (``learning_rate``, ``apply_multiloss``, ``weighting_double_readout``) are not among what
``config.py`` parses, so they default to nrx_rt's first schedule entry: 1e-3, False, 0.02.
"""
from __future__ import annotations

import argparse
import ctypes
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
                   want_outputs=False, stream=None, workspace=None):
        """Launch ``nrx_train_grad`` on the batch (a ``generator.SlotBatch`` with ``h`` when ``w_chest > 0``): the
        gradient of ``loss_data + w_chest loss_chest`` lands in ``self.g``, the two losses in ``self.loss``
        (device, float64).  Nothing synchronises.  ``want_outputs``: also return ``(llr, h_ref)`` of the last
        readout, in the engine's layouts."""
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
        _lib.check(self._lib.nrx_train_grad(ctypes.byref(self._desc), ctypes.byref(io), ws.data_ptr(), ws.numel(),
                                            stream_of(self.w, stream)))
        return out

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


def main(argv=None):
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
    a = ap.parse_args(argv)
    evaluate.check_arguments(ap, a)
    if a.steps < 0 or a.ebno_db_max < a.ebno_db_min:
        ap.error("-steps must be >= 0 and -ebno_db_max >= -ebno_db_min")

    import torch
    from . import weights as W
    from .config import get_config
    from .generator import SlotGenerator, count_errors, ebno_to_no
    from .receiver import compute_pe, spec_for
    device = a.gpu if a.gpu is not None else 0
    torch.cuda.set_device(device)
    cfg = get_config(a.config_name)
    spec = spec_for(cfg)
    params, u, _ = evaluate.generator_params(a, cfg)
    max_active = params.num_active
    init = W.load(cfg.label) if a.init == "shipped" else W.seeded(spec, a.seed) if a.init == "seeded" \
        else W.load_file(a.init)
    tr = Trainer(spec, init, device=device)
    gen = SlotGenerator(params, device=device, want_h=True)
    held = SlotGenerator(params, device=device, want_h=True)       # its own buffers: the batch stays
    dev = torch.device("cuda", device)
    pe = torch.from_numpy(compute_pe(params.num_tx, params.num_subcarriers, params.dmrs_symbols,
                                     params.cdm_group)).to(dev)
    nd = len(params.dmrs_symbols)
    eval_ebno = a.eval_ebno_db if a.eval_ebno_db is not None else 0.5 * (a.ebno_db_min + a.ebno_db_max)
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

    rng = np.random.default_rng(a.seed)
    print(f"step 0  held-out BER {held_out_ber():.4e} at {eval_ebno:g} dB", flush=True)
    for k in range(a.steps):
        ebno = rng.uniform(a.ebno_db_min, a.ebno_db_max)
        params.num_active = int(rng.integers(1, max_active + 1))
        sb = gen(a.batch_size, ebno_to_no(float(ebno), nd), slot_offset=k * a.batch_size)
        ld, lc = tr.grad(sb, pe, multiloss=a.apply_multiloss, w_chest=a.weighting_double_readout,
                         dmrs_symbols=params.dmrs_symbols)
        tr.step(lr=a.learning_rate)
        if (k + 1) % a.eval_every == 0 or k + 1 == a.steps:
            print(f"step {k + 1}  loss_data {ld:.5f}  loss_chest {lc:.5f}  held-out BER {held_out_ber():.4e}",
                  flush=True)
    if a.out:
        W.save(a.out, tr.weights())
    return tr


if __name__ == "__main__":
    main()
