"""The binding layer the wrappers share (neural_rx_amd/_call.py), on the host: descriptor fillers on the
real ``_lib`` structs, the tensor check, and the workspace buffer on ``device="cpu"``."""
import ctypes

import pytest
import torch

from neural_rx_amd import _call, _lib

GRID_STRUCTS = [c for c in vars(_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure)
                and hasattr(c, "num_subcarriers")]
ANT_STRUCTS = [c for c in GRID_STRUCTS if hasattr(c, "num_rx_ant")]
MCS_STRUCTS = [c for c in GRID_STRUCTS if hasattr(c, "mcs_bits")]
DMRS_STRUCTS = [c for c in GRID_STRUCTS if hasattr(c, "cdm_group")]


def test_the_structs_the_fillers_serve():
    names = lambda cs: {c.__name__ for c in cs}   # noqa: E731
    assert names(MCS_STRUCTS) == {"nrx_gen_desc", "nrx_count_io", "nrx_lmmse_io", "nrx_kbest_io", "nrx_llr_stats_io",
                                  "nrx_ldpc_gather_io"}
    assert names(DMRS_STRUCTS) == {"nrx_gen_desc", "nrx_cfo_io", "nrx_ls_io", "nrx_chest_io", "nrx_chest3_io"}
    assert len(GRID_STRUCTS) == 14 and len(ANT_STRUCTS) == 10


@pytest.mark.parametrize("cls", GRID_STRUCTS, ids=lambda c: c.__name__)
def test_fill_grid(cls):
    io = cls()
    _call.fill_grid(io, 3, 2, 24, 14)
    assert (io.batch, io.num_tx, io.num_subcarriers, io.num_symbols) == (3, 2, 24, 14)
    if cls in ANT_STRUCTS:
        assert io.num_rx_ant == 0
        _call.fill_grid(io, 5, 1, 12, 14, 4)
        assert (io.batch, io.num_tx, io.num_subcarriers, io.num_symbols, io.num_rx_ant) == (5, 1, 12, 14, 4)


@pytest.mark.parametrize("cls", MCS_STRUCTS, ids=lambda c: c.__name__)
def test_fill_mcs(cls):
    io = cls()
    _call.fill_mcs(io, (2, 4, 6))
    assert io.num_mcs == 3 and list(io.mcs_bits) == [2, 4, 6, 0, 0, 0, 0, 0] and io.dmrs_symbol_mask == 0
    _call.fill_mcs(io, [4], dmrs_symbols=(2, 11))
    assert io.num_mcs == 1 and io.mcs_bits[0] == 4 and io.dmrs_symbol_mask == (1 << 2) | (1 << 11)
    _call.fill_mcs(io, (4,), dmrs_symbols=(2, 3, 10, 11))
    assert io.dmrs_symbol_mask == 0b110000001100
    if hasattr(cls, "bits_stride"):
        assert io.bits_stride == 0
        _call.fill_mcs(io, (4,), bits_stride=6)
        assert io.bits_stride == 6
    if hasattr(cls, "num_heads"):
        assert io.num_heads == 0
        _call.fill_mcs(io, (4,), num_heads=2)
        assert io.num_heads == 2
    # nine widths: the array holds eight, the count says nine, so the C check refuses the call
    io = cls()
    _call.fill_mcs(io, range(1, 10), dmrs_symbols=(2,))
    assert io.num_mcs == 9 and list(io.mcs_bits) == list(range(1, 9)) and io.dmrs_symbol_mask == 4


@pytest.mark.parametrize("cls", DMRS_STRUCTS, ids=lambda c: c.__name__)
def test_fill_dmrs(cls):
    io = cls()
    _call.fill_dmrs(io, (2, 11), (0, 1, 1, 0), 3)
    assert io.num_dmrs_symbols == 2 and list(io.dmrs_symbols) == [2, 11, 0, 0]
    assert list(io.cdm_group) == [0, 1, 1] + [0] * 13            # the first num_tx ports only
    # five symbols: four written, the count says five
    io = cls()
    _call.fill_dmrs(io, (1, 2, 3, 4, 5), (1,), 1)
    assert io.num_dmrs_symbols == 5 and list(io.dmrs_symbols) == [1, 2, 3, 4] and io.cdm_group[0] == 1
    # seventeen ports: sixteen groups written, num_tx (fill_grid's) says seventeen
    io = cls()
    _call.fill_grid(io, 1, 17, 12, 14)
    _call.fill_dmrs(io, (2,), [1] * 17, 17)
    assert io.num_tx == 17 and list(io.cdm_group) == [1] * 16


def test_ptr_and_ref():
    t = torch.zeros(4)
    assert _call.ptr(t) == t.data_ptr() and _call.ptr(None) is None
    io = _lib.nrx_cov_io()
    assert _call.ref(None) is None
    io.batch = 7
    assert ctypes.cast(_call.ref(io), ctypes.POINTER(_lib.nrx_cov_io)).contents.batch == 7
    assert _call.torch() is torch
    assert _call.stream_of(t, 1234) == 1234          # a given stream is passed on, no device asked


def test_require_accepts_and_returns():
    t = torch.zeros((2, 3), dtype=torch.float32)
    assert _call.require("t", t) is t
    assert _call.require("t", t, (2, 3), torch.float32, "cpu") is t
    assert _call.require("t", t, [2, 3], device=torch.device("cpu")) is t
    assert _call.require("t", t.t(), (3, 2), contiguous=False).shape == (3, 2)


@pytest.mark.parametrize("kw,word", [
    (dict(shape=(3, 2)), "(3, 2)"), (dict(shape=(2, 3, 1)), "(2, 3, 1)"), (dict(dtype=torch.float64), "float64"),
    (dict(dtype=torch.uint8), "uint8"), (dict(device="meta"), "meta"),
])
def test_require_refuses(kw, word):
    t = torch.zeros((2, 3), dtype=torch.float32)
    with pytest.raises(ValueError, match="t must be") as e:
        _call.require("t", t, **kw)
    assert word in str(e.value) and "got float32 (2, 3) on cpu" in str(e.value)


def test_require_refuses_non_contiguous():
    t = torch.zeros((2, 3), dtype=torch.float32).t()
    with pytest.raises(ValueError, match="contiguous"):
        _call.require("t", t, (3, 2), torch.float32)
    with pytest.raises(ValueError, match="contiguous"):
        _call.require("t", t)


def test_workspace_exact_grow_only_and_reused():
    ws = _call.Workspace()
    assert ws.buf is None
    a = ws.get(1000, "cpu")
    assert a.numel() == 1000 and a.dtype == torch.uint8 and a.device.type == "cpu" and ws.buf is a
    assert ws.get(1000, "cpu") is a and ws.get(10, "cpu") is a and ws.get(0, "cpu") is a     # never shrinks
    b = ws.get(1001, "cpu")
    assert b is not a and b.numel() == 1001 and ws.buf is b                                  # exact, not rounded
    assert ws.get(1000, torch.device("cpu")) is b
    c = ws.get(5, "meta")                                                                    # another device
    assert c.device.type == "meta" and c.numel() == 5 and ws.buf is c


def test_workspace_callers_tensor():
    ws = _call.Workspace()
    own = ws.get(64, "cpu")
    given = torch.full((8,), 7, dtype=torch.uint8)
    assert ws.get(1 << 20, "cpu", given) is given         # passed on as it is: the C call checks its size
    assert ws.buf is own and own.numel() == 64 and (given == 7).all()
    for bad in (torch.zeros(8, dtype=torch.int8), torch.zeros(8, dtype=torch.float32),
                torch.zeros((8, 2), dtype=torch.uint8)[:, 0], torch.zeros(8, dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError, match="workspace must be a contiguous uint8 tensor on cpu"):
            ws.get(8, "cpu", bad)
    assert ws.buf is own


def test_workspace_size_query_and_keyed_cache():
    calls = []

    def size_fn(a, b, out):
        calls.append((a, b))
        ctypes.cast(out, ctypes.POINTER(ctypes.c_size_t)).contents.value = 100 * a + b
        return _lib.NRX_OK

    ws = _call.Workspace()
    assert ws.size(size_fn, 1, 2) == 102 and ws.size(size_fn, 1, 2) == 102 and len(calls) == 2     # no key: asked
    assert ws.size(size_fn, 3, 4, key="x") == 304 and ws.size(size_fn, 9, 9, key="x") == 304       # once per key
    assert ws.size(size_fn, 5, 6, key=("y", 1)) == 506 and ws.size(size_fn, 5, 6, key=("y", 1)) == 506
    assert calls == [(1, 2), (1, 2), (3, 4), (5, 6)]
    with pytest.raises(_lib.NRXError):
        ws.size(lambda out: _lib.NRX_ERR_INVALID_ARG, key="bad")
    assert ws.size(size_fn, 7, 8, key="bad") == 708                                                # a failure is not cached
