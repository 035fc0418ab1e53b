"""The fp64 oracle with the engine's f16 storage roundings: a reference for how far an f16
forward may sit from the fp64 oracle (test infrastructure only).

``f16_rounded_oracle(case)`` runs ``oracle.cgnn_ref.cgnn_forward`` with its ``sepconv`` and
``dense`` swapped for the "act+w+dw-math f16" model of tools/fp16_sensitivity.py:

* every stored activation (a layer's input, the depthwise output) and every kernel (depthwise,
  pointwise, dense; not the biases, which the engine keeps in f32) is rounded to f16;
* the depthwise 3x3 is summed in f16 in the kernels' order (``P16T::dw_row``,
  nrx_device.inc): the centre column j = 1 first, i = 0, 1, 2, then the j = 0 column, then the
  j = 2 column, each step one fused multiply-add rounded once (the product of two f16 values
  is exact in f64, so ``rnd(acc + w * x)`` rounds once);
* the pointwise / dense matmul and the bias run in f64 (the engine accumulates in f32 on the
  MFMA, which this model does not reproduce).

With ``rnd`` the identity and ``dw_order="oracle"`` the swapped functions are the oracle's own
arithmetic and the result equals ``run_oracle(case)`` bit for bit (tests/test_gpu_topologies.py
checks that on the CPU).  The originals are restored in a ``finally`` block.
"""
from __future__ import annotations

import numpy as np

from oracle import cgnn_ref

# (i along F, j along T) taps in the order the kernels accumulate them / the oracle's loops do
KERNEL_ORDER = ((0, 1), (1, 1), (2, 1), (0, 0), (1, 0), (2, 0), (0, 2), (1, 2), (2, 2))
ORACLE_ORDER = tuple((i, j) for i in range(3) for j in range(3))


def r16(x):
    return np.asarray(x).astype(np.float16).astype(np.float64)


def _rounded_layers(rnd, order):
    def sepconv(x, w, relu):
        x = rnd(np.asarray(x, np.float64))
        n, f, t, c = x.shape
        xp = np.zeros((n, f + 2, t + 2, c), np.float64)
        xp[:, 1:-1, 1:-1] = x
        dw = rnd(w.dw[..., 0].astype(np.float64))
        d = np.zeros_like(x)
        for i, j in order:
            d = rnd(d + dw[i, j] * xp[:, i:i + f, j:j + t, :])
        out = rnd(d) @ rnd(w.pw[0, 0].astype(np.float64)) + w.b.astype(np.float64)
        return np.maximum(out, 0) if relu else out

    def dense(x, w, relu):
        x = np.asarray(x, np.float64)
        out = rnd(x) @ rnd(w.w.astype(np.float64)) + w.b.astype(np.float64)
        return np.maximum(out, 0) if relu else out

    return sepconv, dense


def f16_rounded_oracle(case, rnd=r16, dw_order="kernel"):
    """``tests.helpers.run_oracle(case)`` (fp64) under the f16 rounding model above."""
    order = {"kernel": KERNEL_ORDER, "oracle": ORACLE_ORDER}[dw_order]
    orig = cgnn_ref.sepconv, cgnn_ref.dense
    cgnn_ref.sepconv, cgnn_ref.dense = _rounded_layers(rnd, order)
    try:
        w = cgnn_ref.split_keras_weights(case.weights, case.spec)
        return cgnn_ref.cgnn_forward(case.y, case.pe, case.h_hat, case.active, case.mcs_mask, w,
                                     case.spec, num_it=case.num_it, dtype=np.float64)
    finally:
        cgnn_ref.sepconv, cgnn_ref.dense = orig
