"""The soft-metric entry points of include/nrx.h (nrx_llr_stats, nrx_chest_nmse and their
workspace-size calls): exports, struct layouts and the argument checks, which run before the first
HIP call -- so their status codes are checked here without a GPU."""
import ctypes
import os

import pytest

from neural_rx_amd import _lib

INVALID_ARG, SHAPE, WORKSPACE = -1, -2, -6


@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def _llr_io(**kw):
    """A valid descriptor whose pointers are non-null but never dereferenced on the host: every
    case below must be rejected before the first HIP call."""
    io = _lib.nrx_llr_stats_io()
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = 2, 2, 12, 14
    io.num_heads, io.bits_stride, io.num_mcs = 1, 6, 3
    io.mcs_bits[0], io.mcs_bits[1], io.mcs_bits[2] = 2, 4, 6
    io.dmrs_symbol_mask = (1 << 2) | (1 << 11)
    io.num_scales = 2
    io.scales[0], io.scales[1] = 1.0, 2.0
    io.llr = io.bits = io.mcs = io.active = io.loss = io.cnt = io.nonfinite = 4096
    for k, v in kw.items():
        if k.startswith("mcs_bits"):
            io.mcs_bits[int(k[8:])] = v
        elif k.startswith("scales"):
            io.scales[int(k[6:])] = v
        else:
            setattr(io, k, v)
    return io


def _nmse_io(**kw):
    io = _lib.nrx_nmse_io()
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = 2, 2, 12, 14
    io.num_rx_ant, io.symbol_mask = 4, 0
    io.h_est = io.h_true = io.active = io.err = io.ref = io.items = 4096
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def test_exports_and_bindings(lib):
    for s in ("nrx_llr_stats_workspace_size", "nrx_llr_stats", "nrx_nmse_workspace_size", "nrx_chest_nmse"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    # nrx_llr_stats_io: 17 int32 + 4 bytes of padding, 16 doubles, 7 pointers
    assert ctypes.sizeof(_lib.nrx_llr_stats_io) == 18 * 4 + 16 * 8 + 7 * 8
    assert _lib.nrx_llr_stats_io.num_scales.offset == 64 and _lib.nrx_llr_stats_io.scales.offset == 72
    assert _lib.nrx_llr_stats_io.llr.offset == 200
    # the leading fields are those of nrx_count_io, in its order
    cnt = [n for n, _ in _lib.nrx_count_io._fields_][:9]
    assert [n for n, _ in _lib.nrx_llr_stats_io._fields_][:9] == cnt
    assert ctypes.sizeof(_lib.nrx_nmse_io) == 6 * 4 + 6 * 8 and _lib.nrx_nmse_io.h_est.offset == 24
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nrx.h")).read()
    assert f"#define NRX_SOFT_STRIP {_lib.SOFT_STRIP}\n" in header


def test_api_version_is_unchanged(lib):
    assert lib.nrx_api_version() == 7


LLR_CASES = [
    (dict(llr=None), INVALID_ARG, b"null"), (dict(bits=None), INVALID_ARG, b"null"),
    (dict(active=None), INVALID_ARG, b"null"), (dict(loss=None), INVALID_ARG, b"null"),
    (dict(cnt=None), INVALID_ARG, b"null"), (dict(nonfinite=None), INVALID_ARG, b"null"),
    (dict(num_scales=0), INVALID_ARG, b"num_scales"), (dict(num_scales=17), INVALID_ARG, b"num_scales"),
    (dict(num_scales=-1), INVALID_ARG, b"num_scales"),
    (dict(scales0=0.0), INVALID_ARG, b"scales"), (dict(scales1=-1.0), INVALID_ARG, b"scales"),
    (dict(scales0=float("nan")), INVALID_ARG, b"scales"), (dict(scales1=float("inf")), INVALID_ARG, b"scales"),
    (dict(mcs_bits1=0), INVALID_ARG, b"mcs_bits"), (dict(mcs_bits0=9), INVALID_ARG, b"mcs_bits"),
    (dict(dmrs_symbol_mask=1 << 14), INVALID_ARG, b"dmrs_symbol_mask"),
    (dict(dmrs_symbol_mask=-1), INVALID_ARG, b"dmrs_symbol_mask"),
    (dict(num_symbols=12), SHAPE, b"num_symbols"), (dict(batch=0), SHAPE, b"batch"),
    (dict(batch=65536), SHAPE, b"batch"), (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"),
    (dict(num_subcarriers=3301), SHAPE, b"num_subcarriers"), (dict(num_tx=0), SHAPE, b"num_tx"),
    (dict(num_tx=17), SHAPE, b"num_tx"), (dict(num_mcs=0), SHAPE, b"num_mcs"), (dict(num_mcs=9), SHAPE, b"num_mcs"),
    (dict(bits_stride=5), SHAPE, b"bits_stride"), (dict(num_heads=2), SHAPE, b"num_heads"),
    (dict(num_heads=0), SHAPE, b"num_heads"), (dict(num_heads=4), SHAPE, b"num_heads"),
]


@pytest.mark.parametrize("kw,code,word", LLR_CASES)
def test_llr_stats_argument_checks(lib, kw, code, word):
    io = _llr_io(**kw)
    assert lib.nrx_llr_stats(ctypes.byref(io), 4096, 1 << 40, None) == code
    assert word in lib.nrx_last_error()
    n = ctypes.c_size_t(0)
    assert lib.nrx_llr_stats_workspace_size(ctypes.byref(io), ctypes.byref(n)) == code


NMSE_CASES = [
    (dict(h_est=None), INVALID_ARG, b"null"), (dict(h_true=None), INVALID_ARG, b"null"),
    (dict(active=None), INVALID_ARG, b"null"), (dict(err=None), INVALID_ARG, b"null"),
    (dict(ref=None), INVALID_ARG, b"null"), (dict(items=None), INVALID_ARG, b"null"),
    (dict(symbol_mask=1 << 14), INVALID_ARG, b"symbol_mask"), (dict(symbol_mask=-4), INVALID_ARG, b"symbol_mask"),
    (dict(num_symbols=13), SHAPE, b"num_symbols"), (dict(batch=0), SHAPE, b"batch"),
    (dict(batch=65536), SHAPE, b"batch"), (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"),
    (dict(num_subcarriers=3301), SHAPE, b"num_subcarriers"), (dict(num_tx=0), SHAPE, b"num_tx"),
    (dict(num_tx=17), SHAPE, b"num_tx"), (dict(num_rx_ant=0), SHAPE, b"num_rx_ant"),
    (dict(num_rx_ant=17), SHAPE, b"num_rx_ant"),
]


@pytest.mark.parametrize("kw,code,word", NMSE_CASES)
def test_nmse_argument_checks(lib, kw, code, word):
    io = _nmse_io(**kw)
    assert lib.nrx_chest_nmse(ctypes.byref(io), 4096, 1 << 40, None) == code
    assert word in lib.nrx_last_error()
    n = ctypes.c_size_t(0)
    assert lib.nrx_nmse_workspace_size(ctypes.byref(io), ctypes.byref(n)) == code


def test_null_io_workspace_and_bytes(lib):
    n = ctypes.c_size_t(0)
    assert lib.nrx_llr_stats(None, 4096, 1 << 40, None) == INVALID_ARG
    assert lib.nrx_llr_stats_workspace_size(None, ctypes.byref(n)) == INVALID_ARG
    assert lib.nrx_chest_nmse(None, 4096, 1 << 40, None) == INVALID_ARG
    assert lib.nrx_nmse_workspace_size(None, ctypes.byref(n)) == INVALID_ARG
    io, nio = _llr_io(), _nmse_io()
    assert lib.nrx_llr_stats_workspace_size(ctypes.byref(io), None) == INVALID_ARG
    assert lib.nrx_nmse_workspace_size(ctypes.byref(nio), None) == INVALID_ARG
    assert lib.nrx_llr_stats(ctypes.byref(io), None, 1 << 40, None) == INVALID_ARG
    assert b"workspace" in lib.nrx_last_error()
    assert lib.nrx_chest_nmse(ctypes.byref(nio), None, 1 << 40, None) == INVALID_ARG
    assert lib.nrx_llr_stats(ctypes.byref(io), 4100, 1 << 40, None) == INVALID_ARG
    assert b"aligned" in lib.nrx_last_error()
    assert lib.nrx_chest_nmse(ctypes.byref(nio), 4100, 1 << 40, None) == INVALID_ARG
    # mcs may be NULL (= MCS 0): the call passes the checks and stops at the workspace size
    io.mcs = None
    assert lib.nrx_llr_stats(ctypes.byref(io), 4096, 8, None) == WORKSPACE


def test_small_workspace_is_reported(lib):
    io, nio = _llr_io(), _nmse_io()
    n = ctypes.c_size_t(0)
    assert lib.nrx_llr_stats_workspace_size(ctypes.byref(io), ctypes.byref(n)) == 0
    assert lib.nrx_llr_stats(ctypes.byref(io), 4096, n.value - 1, None) == WORKSPACE
    assert b"workspace too small" in lib.nrx_last_error() and str(n.value).encode() in lib.nrx_last_error()
    assert lib.nrx_nmse_workspace_size(ctypes.byref(nio), ctypes.byref(n)) == 0
    assert lib.nrx_chest_nmse(ctypes.byref(nio), 4096, n.value - 1, None) == WORKSPACE
    assert b"workspace too small" in lib.nrx_last_error()


def _sizes(lib, **kw):
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    io = _llr_io(**{k: v for k, v in kw.items()})
    assert lib.nrx_llr_stats_workspace_size(ctypes.byref(io), ctypes.byref(n)) == 0
    nio = _nmse_io(**{k: v for k, v in kw.items() if k != "num_scales"})
    assert lib.nrx_nmse_workspace_size(ctypes.byref(nio), ctypes.byref(m)) == 0
    return n.value, m.value


def test_workspace_grows_with_items(lib):
    """one partial record per (slot, user, strip of NRX_SOFT_STRIP subcarriers): [8][S] f64 + two [8]
    i64 for the LLRs, two f64 for the NMSE"""
    FS = _lib.SOFT_STRIP
    base = _sizes(lib)
    assert base == (2 * 2 * 1 * (8 * 2 + 16) * 8, 2 * 2 * 1 * 16)
    assert _sizes(lib, batch=4) == (2 * base[0], 2 * base[1])
    assert _sizes(lib, num_tx=6) == (3 * base[0], 3 * base[1])
    assert _sizes(lib, num_subcarriers=FS) == base                       # still one strip
    assert _sizes(lib, num_subcarriers=FS + 1) == (2 * base[0], 2 * base[1])
    assert _sizes(lib, num_subcarriers=2 * FS + 5) == (3 * base[0], 3 * base[1])
    assert _sizes(lib, num_scales=1)[0] == 2 * 2 * (8 + 16) * 8
