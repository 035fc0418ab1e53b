"""The variant of the one-item column kernels the plan picks (``StagePlan::variant``, csrc/nrx_dispatch.hip), without a
GPU: ``nrx_debug_forward_plan`` / ``nrx_debug_forward_plan_io`` report it as word 14 of every stage record (the words
tests/test_forward_plan.py reads keep their meaning).

A lean variant holds as compile-time constants what is uniform over the launch: one strip, the slot norm fused, a model
with h_hat, one StateInit (masking or one MCS), one LLR head of bits_max = 4, 2A = 8, one item per workgroup; the
readout is lean with (1) or without (2) the ChEst store.  The plan must pick it exactly when every fact holds, and the
generic variant (0) as soon as one fails."""
import ctypes
import dataclasses

import pytest

from neural_rx_amd import _lib
from neural_rx_amd.config import get_config, spec_from_config

REC = 16
KIND, TAIL, ONE, VARIANT = 3, 5, 7, 14
COL = 2
TAIL_READOUT_WB = 2
GENERIC, LEAN, LEAN_NO_HREF = 0, 1, 2
DEFAULT_MASK = 29
WIDE = DEFAULT_MASK | 64
H_REF, MCS_MASK = 1, 2


def lib_():
    return _lib.load()


def stages(lib, spec, users, prbs, batch, mask=DEFAULT_MASK, io_flags=0, num_it=None):
    fn = lib.nrx_debug_forward_plan_io
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(_lib.nrx_desc), ctypes.POINTER(_lib.nrx_shape)] + [ctypes.c_int32] * 7 + [
        ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]
    desc = _lib.make_desc(spec)
    sh = _lib.nrx_shape(batch, users, 12 * prbs, 14)
    cap = REC * 17 * 64
    out = (ctypes.c_int32 * cap)()
    # fused 0: the three launches (whose stages the variants are)
    n = fn(ctypes.byref(desc), ctypes.byref(sh), 0, num_it or spec.num_it, mask, 0, 256, 8, io_flags, out, cap)
    assert 0 < n <= cap and n % REC == 0, (n, lib.nrx_last_error())
    recs = [list(out[i:i + REC]) for i in range(0, n, REC)]
    return [r for r in recs if r[2] >= 0]


def spec_of(config, ants=4):
    return spec_from_config(get_config(config), ants)


def test_bench_shape_is_lean():
    sp = spec_of("nrx_rt")
    for flags, readout in ((0, LEAN_NO_HREF), (H_REF, LEAN), (MCS_MASK, LEAN_NO_HREF), (H_REF | MCS_MASK, LEAN)):
        st = stages(lib_(), sp, 2, 4, 128, io_flags=flags)
        assert len(st) == 1 + sp.num_it
        assert all(r[KIND] == COL and r[ONE] == 1 for r in st)
        assert [r[VARIANT] for r in st] == [LEAN] * sp.num_it + [readout], (flags, st)
        assert st[-1][TAIL] == TAIL_READOUT_WB


def test_small_shapes_of_the_family_are_lean():
    # the fewest slots the 24-row tier takes by default (beyond the 16-row tier's reach of 256 items), odd batches
    sp = spec_of("nrx_rt")
    for users, prbs, batch in ((2, 4, 43), (1, 4, 129), (2, 4, 127)):
        st = stages(lib_(), sp, users, prbs, batch, io_flags=H_REF)
        assert all(r[KIND] == COL and r[VARIANT] == LEAN for r in st), (users, prbs, batch, st)


def test_strip_stages_have_no_variant():
    # schedule mask 0: strip kernels everywhere
    st = stages(lib_(), spec_of("nrx_rt"), 2, 4, 128, mask=0, io_flags=H_REF)
    assert all(r[KIND] != COL and r[VARIANT] == GENERIC for r in st)


def generic_cases():
    rt = spec_of("nrx_rt")
    return {
        # F = 60: two column strips (a halo, f_start != 0)
        "F=60": (rt, 2, 5, 64, WIDE),
        # Var-IO: two StateInits with mask weights, two LLR heads (the readout is the strip kernel's)
        "var-io": (spec_of("nrx_rt_var_mcs"), 2, 4, 128, DEFAULT_MASK),
        # one 6-bit head
        "bits_max=6": (spec_of("nrx_large_var_mcs_64qam_masking"), 2, 4, 128, DEFAULT_MASK),
        # 16 rx antennas: 2A = 32 (strip StateInit, ch32 updates)
        "2A=32": (spec_of("nrx_rt", 16), 2, 4, 128, DEFAULT_MASK),
        # two LLR heads
        "H=2": (spec_of("nrx_rt_var_mcs"), 2, 4, 64, DEFAULT_MASK),
        # a model that takes no h_hat
        "no h_hat": (dataclasses.replace(rt, use_h_hat=False), 2, 4, 128, DEFAULT_MASK),
        # more items than CUs: the looping kernels
        "items > CUs": (rt, 2, 4, 129, DEFAULT_MASK),
    }


@pytest.mark.parametrize("name", list(generic_cases()))
def test_one_failing_fact_gives_the_generic_variant(name):
    sp, users, prbs, batch, mask = generic_cases()[name]
    for flags in (0, H_REF):
        st = stages(lib_(), sp, users, prbs, batch, mask=mask, io_flags=flags)
        assert any(r[KIND] == COL for r in st), (name, st)
        assert all(r[VARIANT] == GENERIC for r in st), (name, flags, st)


def test_h_ref_only_changes_the_readout():
    sp = spec_of("nrx_rt")
    a = stages(lib_(), sp, 2, 4, 128, io_flags=0)
    b = stages(lib_(), sp, 2, 4, 128, io_flags=H_REF)
    assert [r[:VARIANT] for r in a] == [r[:VARIANT] for r in b]
    assert [r[VARIANT] for r in a[:-1]] == [r[VARIANT] for r in b[:-1]]
    assert (a[-1][VARIANT], b[-1][VARIANT]) == (LEAN_NO_HREF, LEAN)


def test_plan_io_agrees_with_the_plain_call_and_refuses_bad_flags():
    lib = lib_()
    sp = spec_of("nrx_rt")
    st = stages(lib, sp, 2, 4, 128, io_flags=0)
    fn = lib.nrx_debug_forward_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(_lib.nrx_desc), ctypes.POINTER(_lib.nrx_shape)] + [ctypes.c_int32] * 6 + [
        ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]
    desc = _lib.make_desc(sp)
    sh = _lib.nrx_shape(128, 2, 48, 14)
    out = (ctypes.c_int32 * (REC * 8))()
    n = fn(ctypes.byref(desc), ctypes.byref(sh), 0, sp.num_it, DEFAULT_MASK, 0, 256, 8, out, REC * 8)
    assert n == REC * (2 + sp.num_it)
    assert [list(out[i:i + REC]) for i in range(REC, n, REC)] == st
    fio = lib.nrx_debug_forward_plan_io
    for bad in (-1, 4):
        assert fio(ctypes.byref(desc), ctypes.byref(sh), 0, sp.num_it, DEFAULT_MASK, 0, 256, 8, bad, out, REC * 8) < 0
