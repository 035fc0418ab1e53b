"""The byte counts of every ``*_workspace_size`` entry point of include/nrx.h over a table of descriptors, held
against tests/golden/workspace_sizes.json, which tests/golden/make_workspace_sizes.py recorded from the library
before the workspaces were laid out by one carver.  A size is part of the contract: callers allocate it once and
keep the buffer, and the kernels' addresses must stay inside it.

``sizes_cpu`` are the entry points that need no handle (size calls make no HIP call, so no GPU);
``sizes_gpu`` the handle-bound ones.  Size calls only: nothing of these sizes is allocated.  Pointer fields hold
an address that passes the alignment checks and is never dereferenced.
"""
import ctypes
import json
import os

import pytest

from neural_rx_amd import _lib
from neural_rx_amd._call import fill_dmrs, fill_grid, fill_mcs, ref
from neural_rx_amd.cir import SELECT
from neural_rx_amd.config import ModelSpec
from tests.gen_stages import COMBOS, SHAPES, gen_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.json")
PTR = 4096
T = 14
Y_LAYOUTS = {"cgnn": 0, "sionna": 1, "split": 2}
# (batch, num_tx, num_subcarriers); "chunk": an f16 forward workspace beyond the 1 GB range of conv1's row loader,
# which runs in slot chunks: its size is one chunk's (nrx_api.cpp chunk_slots)
FWD_SHAPES = {"tiny": (3, 2, 24), "full": (128, 8, 3276), "chunk": (64, 8, 3276)}


def _size(fn, *args):
    n = ctypes.c_size_t(0)
    rc = fn(*args, ctypes.byref(n))
    assert rc == 0, (rc, _lib.load().nrx_last_error())
    return n.value


def gen_structs(p, batch):
    """(desc, chan, cfo, dmrs, cir, td, tc) of a generator call as SlotGenerator builds them, without a device"""
    chan = cfo = dmrs = cir = None
    if p.correlated:
        chan = _lib.nrx_gen_chan()
        for u, (delay, doppler) in enumerate(p.profiles()):
            chan.max_delay_s[u], chan.max_doppler_hz[u] = delay, doppler
        chan.rx_mix = PTR
    if p.cfo_hz is not None:
        cfo = _lib.nrx_gen_cfo()
        for u, hz in enumerate(p.cfo_per_port()):
            cfo.cfo_hz[u] = hz
        cfo.constant, cfo.fft_size, cfo.h_with_phase = int(p.cfo_constant), int(p.fft_size), int(p.h_with_phase)
    if p.dmrs is not None:
        dmrs = _lib.nrx_gen_dmrs()
        for u in range(p.num_tx):
            dmrs.focc[u], dmrs.tocc[u] = p.dmrs.focc[u], p.dmrs.tocc[u]
        dmrs.despread_f, dmrs.despread_t = int(p.dmrs.despread_f), int(p.dmrs.despread_t)
    if p.cir is not None:
        ds = p.cir.dataset
        cir = _lib.nrx_gen_cir()
        cir.num_examples, cir.num_paths, cir.num_time_steps = ds.num_examples, ds.num_paths, ds.num_time_steps
        cir.select, cir.normalize, cir.f_offset = SELECT[p.cir.select], 1, p.cir.offset(p.num_subcarriers)
        cir.a = cir.tau = PTR
    td = p.td.struct(p.num_tx) if p.td is not None else None
    tc = p.tc.struct() if p.tc is not None else None
    return p.desc(batch, 0.0), chan, cfo, dmrs, cir, td, tc


def sizes_cpu(lib):
    out = {}
    for shape in SHAPES:
        for combo in COMBOS:
            d, chan, cfo, dmrs, cir, td, tc = gen_structs(*gen_params(combo, shape))
            d, rest = ref(d), [ref(s) for s in (cfo, dmrs, cir, td)]
            key = f"gen/{shape}/{combo}/"
            out[key + "tc"] = _size(lib.nrx_gen_workspace_size_tc, d, ref(chan), *rest, ref(tc))
            # the older entry points are that call with fewer blocks: each one that can state the combination
            # (chan changes no size: those without it take the desc's scalars)
            older = ("nrx_gen_workspace_size", "nrx_gen_workspace_size_cfo", "nrx_gen_workspace_size_dmrs",
                     "nrx_gen_workspace_size_cir", "nrx_gen_workspace_size_td")
            for k, name in enumerate(older):
                if tc is None and all(s is None for s in rest[k:]):
                    out[key + (name[len("nrx_gen_workspace_size_"):] or "plain")] = _size(getattr(lib, name), d, *rest[:k])
        B, U, F, A = (SHAPES[shape][k] for k in ("batch", "num_tx", "num_subcarriers", "num_rx_ant"))
        io = _lib.nrx_kbest_io()
        fill_grid(io, B, U, F, T, A)
        fill_mcs(io, (2, 4, 6), (2, 11), bits_stride=6)
        io.k, io.no, io.err_var, io.llr_clip = 16, 0.1, 0.0, 20.0
        io.y = io.h = io.active = io.llr = PTR
        out[f"kbest/{shape}"] = _size(lib.nrx_kbest_workspace_size, ref(io))
        for name, cls in (("cov", _lib.nrx_cov_io), ("cov_space", _lib.nrx_cov_space_io)):
            io = cls()
            fill_grid(io, B, U, F, T, A)
            io.h = io.acc = PTR
            out[f"{name}/{shape}"] = _size(getattr(lib, f"nrx_{name}_workspace_size"), ref(io))
        io = _lib.nrx_chest3_io()
        fill_grid(io, B, U, F, T, A)
        fill_dmrs(io, (2, 3, 10, 11), [u % 2 for u in range(U)], U)
        out[f"chest3/{shape}"] = _size(lib.nrx_chest3_workspace_size, ref(io))
        io = _lib.nrx_llr_stats_io()
        fill_grid(io, B, U, F, T)
        fill_mcs(io, (2, 4, 6), (2, 11), bits_stride=6, num_heads=3)
        io.num_scales = 5
        for k in range(5):
            io.scales[k] = 0.5 + 0.25 * k
        io.llr = io.bits = io.active = io.loss = io.cnt = io.nonfinite = PTR
        out[f"llr_stats/{shape}"] = _size(lib.nrx_llr_stats_workspace_size, ref(io))
        io = _lib.nrx_nmse_io()
        fill_grid(io, B, U, F, T, A)
        io.h_est = io.h_true = io.active = io.err = io.ref = io.items = PTR
        out[f"nmse/{shape}"] = _size(lib.nrx_nmse_workspace_size, ref(io))
    # training takes at most 2^24 positions: the full slot with 32 slots of 8 users is 11.7 M
    for shape, (B, U, F, A) in (("tiny", (3, 2, 24, 2)), ("full", (32, 8, 3276, 16))):
        for name, masking, multiloss in (("masked", True, 0), ("heads_multiloss", False, 1)):
            d = _lib.make_desc(ModelSpec(num_rx_ant=A, d_s=56, num_it=2, bits=(2, 4), masking=masking, use_h_hat=True))
            io = _lib.nrx_train_io()
            io.shape = _lib.nrx_shape(B, U, F, T)
            io.num_it, io.dmrs_symbol_mask, io.multiloss, io.bits_stride, io.w_chest = 2, (1 << 2) | (1 << 11), multiloss, 4, 0.02
            io.y = io.pe = io.h_hat = io.active = io.bits = io.h = io.weights = io.grad = io.loss = PTR
            out[f"train/{shape}/{name}"] = _size(lib.nrx_train_workspace_size, ref(d), ref(io))
    return out


def sizes_gpu(lib):
    from neural_rx_amd import weights as W
    from neural_rx_amd.config import get_config, spec_from_config
    from neural_rx_amd.ldpc import Decoder, named_code
    from neural_rx_amd.receiver import CGNNEngine
    out = {}
    eng = CGNNEngine(spec_from_config(get_config("nrx_rt")), W.seeded(spec_from_config(get_config("nrx_rt")), seed=5))
    for name, (B, U, F) in FWD_SHAPES.items():
        s = _lib.nrx_shape(B, U, F, T)
        for pname, prec in (("f16", _lib.NRX_PREC_F16), ("f32x", _lib.NRX_PREC_F32X)):
            out[f"forward/{name}/{pname}"] = _size(lib.nrx_workspace_size, eng._h, ref(s), prec)
            for lname, layout in Y_LAYOUTS.items():
                out[f"forward_ex/{name}/{pname}/{lname}"] = _size(lib.nrx_workspace_size_ex, eng._h, ref(s), prec, layout)
            io = _lib.nrx_aerial_io()
            io.shape, io.num_it, io.precision = s, 1, prec
            io.num_dmrs_symbols, io.num_dmrs_subcarriers = 2, 6
            out[f"aerial/{name}/{pname}"] = _size(lib.nrx_aerial_workspace_size, eng._h, ref(io))
    eng.close()
    # r12 at z = 8: the messages fit in LDS next to APP (a constant workspace); r23 at z = 384: (36 + 108) 384 f32
    # do not, and the messages live in the workspace
    for code, z in (("r12", 8), ("r23", 384)):
        dec = Decoder(named_code(code, z))
        for num_cw in (1, 3, 1 << 12):
            io = _lib.nrx_ldpc_io()
            io.num_cw, io.num_iter, io.cn_type, io.early_stop, io.ms_scale, io.llr_clip = num_cw, 20, 0, 1, 0.75, 20.0
            io.llr_in = io.hard = io.iters = io.parity_ok = PTR
            out[f"ldpc/{code}_z{z}/{num_cw}"] = _size(lib.nrx_ldpc_workspace_size, dec._h, ref(io))
    assert out["ldpc/r12_z8/3"] == out["ldpc/r12_z8/1"] and out["ldpc/r23_z384/3"] == 3 * out["ldpc/r23_z384/1"]
    return out


@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)


def _same(got, want):
    assert sorted(got) == sorted(want), "the table and its recording list different cases: record again"
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, f"(now, recorded): {diff}"


def test_sizes_without_a_handle(lib, golden):
    _same(sizes_cpu(lib), golden["cpu"])


def test_the_table_covers_every_stage_combination_at_both_shapes(golden):
    gen = {k for k in golden["cpu"] if k.startswith("gen/") and k.endswith("/tc")}
    assert gen == {f"gen/{s}/{c}/tc" for s in SHAPES for c in COMBOS} and len(COMBOS) == 14
    # every stage grows the workspace it is added to
    g = {k[4:-3]: v for k, v in golden["cpu"].items() if k in gen}
    for s in SHAPES:
        for small, big in (("none", "cfo"), ("none", "dmrs"), ("cfo", "cfo_dmrs"), ("none", "cir1"), ("none", "td"),
                           ("td", "td_dmrs"), ("td", "td_cir"), ("none", "tc"), ("tc", "tc_dmrs")):
            assert g[f"{s}/{small}"] < g[f"{s}/{big}"], (s, small, big)
        assert g[f"{s}/none"] == g[f"{s}/chan"] and g[f"{s}/tc"] == g[f"{s}/tc_chan"] and g[f"{s}/cir1"] == g[f"{s}/cir14"]


@pytest.mark.gpu
def test_sizes_of_the_handle_bound_entry_points(golden):
    got = sizes_gpu(_lib.load())
    _same(got, golden["gpu"])
    # the chunked f16 forward stays below the row loader's range, the unchunked f32x one does not
    assert got["forward/chunk/f16"] < 1 << 30 < got["forward/chunk/f32x"]
