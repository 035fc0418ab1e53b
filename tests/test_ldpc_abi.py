"""The QC-LDPC entry points of include/nrx.h (nrx_ldpc_create / _workspace_size / _decode / _gather /
_count): exports, struct layouts and the argument checks, which run before the first HIP call -- so
their status codes are checked here without a GPU, on a handle created with device = -1."""
import ctypes

import numpy as np
import pytest

from neural_rx_amd import _lib, ldpc

INVALID_ARG, SHAPE, WORKSPACE = -1, -2, -6


@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def _code(mb=4, nb=8, z=8, kb=4, shifts=None):
    if shifts is None:
        shifts = np.full((max(mb, 1), nb), -1, np.int16)    # never empty: the pointer must be non-null
        for i in range(mb):
            shifts[i, i % nb] = 1 % z
            shifts[i, (i + 1) % nb] = 0
        shifts[0, :] = np.where(shifts.max(0) < 0, 0, shifts[0, :])    # no empty column
    shifts = np.ascontiguousarray(shifts, np.int16)
    c = _lib.nrx_ldpc_code()
    c.mb, c.nb, c.z, c.kb = mb, nb, z, kb
    c.shifts = shifts.ctypes.data
    return c, shifts


def _create(lib, *a, **kw):
    c, keep = _code(*a, **kw)
    h = ctypes.c_void_p()
    rc = lib.nrx_ldpc_create(ctypes.byref(c), -1, ctypes.byref(h))
    return rc, h


def _io(**kw):
    io = _lib.nrx_ldpc_io()
    io.num_cw, io.num_iter, io.cn_type, io.early_stop = 3, 20, 0, 1
    io.ms_scale, io.llr_clip = 0.75, 20.0
    io.llr_in = io.skip = io.hard = io.app = io.iters = io.parity_ok = 4096
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def test_exports_layouts_and_version(lib):
    for s in ("nrx_ldpc_create", "nrx_ldpc_destroy", "nrx_ldpc_workspace_size", "nrx_ldpc_decode", "nrx_ldpc_gather",
              "nrx_ldpc_count"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    assert lib.nrx_api_version() == 7
    assert ctypes.sizeof(_lib.nrx_ldpc_code) == 24 and _lib.nrx_ldpc_code.shifts.offset == 16
    assert ctypes.sizeof(_lib.nrx_ldpc_io) == 24 + 6 * 8 and _lib.nrx_ldpc_io.llr_in.offset == 24
    assert ctypes.sizeof(_lib.nrx_ldpc_gather_io) == 80 + 8 * 8 and _lib.nrx_ldpc_gather_io.llr.offset == 80
    assert ctypes.sizeof(_lib.nrx_ldpc_count_io) == 24 + 5 * 8 and _lib.nrx_ldpc_count_io.hard.offset == 24
    # the leading fields of the gather are those of nrx_count_io, in its order
    cnt = [n for n, _ in _lib.nrx_count_io._fields_][:9]
    assert [n for n, _ in _lib.nrx_ldpc_gather_io._fields_][:9] == cnt


CREATE_CASES = [
    (dict(mb=0), SHAPE, b"mb"), (dict(mb=47, nb=68), SHAPE, b"mb"), (dict(nb=1, mb=1), SHAPE, b"nb"),
    (dict(nb=69), SHAPE, b"nb"), (dict(mb=8, nb=8), SHAPE, b"nb must be > mb"), (dict(z=1), SHAPE, b"z"),
    (dict(z=385), SHAPE, b"z"), (dict(kb=0), SHAPE, b"kb"), (dict(kb=8), SHAPE, b"kb"),
]


@pytest.mark.parametrize("kw,code,word", CREATE_CASES)
def test_create_shape_checks(lib, kw, code, word):
    rc, h = _create(lib, **kw)
    assert rc == code and not h.value
    assert word in lib.nrx_last_error()


def test_create_table_checks(lib):
    _, good = _code()
    for mutate, word in (
            (lambda s: s.__setitem__((1, 3), 8), b"shifts"), (lambda s: s.__setitem__((1, 3), -2), b"shifts"),
            (lambda s: s.__setitem__((2, slice(None)), -1), b"row weight"),
            (lambda s: s.__setitem__((2, 3), -1), b"row weight"),
            (lambda s: s.__setitem__((slice(None), 6), -1), b"column weight")):
        s = good.copy()
        mutate(s)
        rc, h = _create(lib, shifts=s)
        assert rc == INVALID_ARG and not h.value and word in lib.nrx_last_error(), word
    # row weight 33
    s = np.zeros((1, 40), np.int16)
    s[0, 33:] = -1
    rc, h = _create(lib, mb=1, nb=40, kb=39, shifts=s)
    assert rc == INVALID_ARG and b"row weight" in lib.nrx_last_error()
    s[0, 32] = -1
    s2 = np.vstack([s, np.zeros((1, 40), np.int16)])
    s2[1, :8] = -1
    rc, h = _create(lib, mb=2, nb=40, kb=38, shifts=s2)
    assert rc == 0 and h.value
    lib.nrx_ldpc_destroy(h)
    c, _ = _code()
    h = ctypes.c_void_p()
    assert lib.nrx_ldpc_create(None, -1, ctypes.byref(h)) == INVALID_ARG
    assert lib.nrx_ldpc_create(ctypes.byref(c), -1, None) == INVALID_ARG
    assert lib.nrx_ldpc_create(ctypes.byref(c), -2, ctypes.byref(h)) == INVALID_ARG
    c.shifts = None
    assert lib.nrx_ldpc_create(ctypes.byref(c), -1, ctypes.byref(h)) == INVALID_ARG
    lib.nrx_ldpc_destroy(None)


DECODE_CASES = [
    (dict(llr_in=None), INVALID_ARG, b"null"), (dict(hard=None), INVALID_ARG, b"null"),
    (dict(iters=None), INVALID_ARG, b"null"), (dict(parity_ok=None), INVALID_ARG, b"null"),
    (dict(num_iter=0), INVALID_ARG, b"num_iter"), (dict(num_iter=101), INVALID_ARG, b"num_iter"),
    (dict(cn_type=2), INVALID_ARG, b"cn_type"), (dict(cn_type=-1), INVALID_ARG, b"cn_type"),
    (dict(early_stop=2), INVALID_ARG, b"early_stop"),
    (dict(cn_type=1, ms_scale=0.0), INVALID_ARG, b"ms_scale"), (dict(cn_type=1, ms_scale=1.5), INVALID_ARG, b"ms_scale"),
    (dict(cn_type=1, ms_scale=float("nan")), INVALID_ARG, b"ms_scale"),
    (dict(llr_clip=0.0), INVALID_ARG, b"llr_clip"), (dict(llr_clip=-1.0), INVALID_ARG, b"llr_clip"),
    (dict(llr_clip=float("inf")), INVALID_ARG, b"llr_clip"), (dict(llr_clip=float("nan")), INVALID_ARG, b"llr_clip"),
    (dict(num_cw=0), SHAPE, b"num_cw"), (dict(num_cw=(1 << 20) + 1), SHAPE, b"num_cw"),
]


@pytest.mark.parametrize("kw,code,word", DECODE_CASES)
def test_decode_argument_checks(lib, kw, code, word):
    rc, h = _create(lib)
    assert rc == 0
    io = _io(**kw)
    assert lib.nrx_ldpc_decode(h, ctypes.byref(io), 4096, 1 << 40, None) == code
    assert word in lib.nrx_last_error()
    n = ctypes.c_size_t(0)
    assert lib.nrx_ldpc_workspace_size(h, ctypes.byref(io), ctypes.byref(n)) == code
    lib.nrx_ldpc_destroy(h)


def test_decode_handle_and_workspace_checks(lib):
    rc, h = _create(lib)
    io = _io()
    n = ctypes.c_size_t(0)
    assert lib.nrx_ldpc_decode(h, None, 4096, 1 << 40, None) == INVALID_ARG
    assert lib.nrx_ldpc_decode(None, ctypes.byref(io), 4096, 1 << 40, None) == INVALID_ARG
    assert b"handle" in lib.nrx_last_error()
    assert lib.nrx_ldpc_workspace_size(None, ctypes.byref(io), ctypes.byref(n)) == INVALID_ARG
    assert lib.nrx_ldpc_workspace_size(h, ctypes.byref(io), None) == INVALID_ARG
    assert lib.nrx_ldpc_decode(h, ctypes.byref(io), None, 1 << 40, None) == INVALID_ARG
    assert b"workspace" in lib.nrx_last_error()
    assert lib.nrx_ldpc_decode(h, ctypes.byref(io), 4100, 1 << 40, None) == INVALID_ARG
    assert b"aligned" in lib.nrx_last_error()
    assert lib.nrx_ldpc_workspace_size(h, ctypes.byref(io), ctypes.byref(n)) == 0 and n.value > 0
    assert lib.nrx_ldpc_decode(h, ctypes.byref(io), 4096, n.value - 1, None) == WORKSPACE
    assert b"workspace too small" in lib.nrx_last_error() and str(n.value).encode() in lib.nrx_last_error()
    # app and skip may be NULL; a handle without a device passes every check and then says so
    io.app = io.skip = None
    assert lib.nrx_ldpc_decode(h, ctypes.byref(io), 4096, n.value, None) == INVALID_ARG
    assert b"no device" in lib.nrx_last_error()
    lib.nrx_ldpc_destroy(h)


def _ws(lib, h, num_cw):
    n = ctypes.c_size_t(0)
    io = _io(num_cw=num_cw)
    assert lib.nrx_ldpc_workspace_size(h, ctypes.byref(io), ctypes.byref(n)) == 0
    return n.value


def test_workspace_is_monotone_in_num_cw(lib):
    """messages that fit in LDS next to APP need no workspace beyond a constant; at the size limits
    (46 x 68, z = 384) they go to the workspace: 4 bytes per edge of the lifted graph and codeword"""
    code = ldpc.named_code("r12", 96)
    c, keep = _code(code.mb, code.nb, code.z, code.kb, code.shifts)
    h = ctypes.c_void_p()
    assert lib.nrx_ldpc_create(ctypes.byref(c), -1, ctypes.byref(h)) == 0
    sizes = [_ws(lib, h, n) for n in (1, 2, 3, 64, 1000, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] == sizes[-1] > 0
    lib.nrx_ldpc_destroy(h)
    rng = np.random.RandomState(0)
    s = np.full((46, 68), -1, np.int16)
    for i in range(46):
        cols = rng.permutation(68)[:3 + i % 17]
        s[i, cols] = rng.randint(0, 384, len(cols))
    s[0, s.max(0) < 0] = 5
    edges = int((s >= 0).sum())
    rc, h = _create(lib, mb=46, nb=68, z=384, kb=22, shifts=s)
    assert rc == 0
    sizes = [_ws(lib, h, n) for n in (1, 2, 3, 64, 1000)]
    assert sizes == [n * edges * 384 * 4 for n in (1, 2, 3, 64, 1000)]
    lib.nrx_ldpc_destroy(h)


def _gather_io(**kw):
    io = _lib.nrx_ldpc_gather_io()
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = 2, 2, 12, 14
    io.num_heads, io.bits_stride, io.num_mcs = 1, 6, 3
    io.mcs_bits[0], io.mcs_bits[1], io.mcs_bits[2] = 2, 4, 6
    io.dmrs_symbol_mask = (1 << 2) | (1 << 11)
    io.num_cw_per_user, io.n_tx, io.n = 2, 100, 128
    io.llr = io.bits = io.mcs = io.active = io.tx_col = io.col_prior = io.llr_in = io.skip = 4096
    for k, v in kw.items():
        if k.startswith("mcs_bits"):
            io.mcs_bits[int(k[8:])] = v
        else:
            setattr(io, k, v)
    return io


GATHER_CASES = [
    (dict(llr=None), INVALID_ARG, b"null"), (dict(bits=None), INVALID_ARG, b"null"),
    (dict(active=None), INVALID_ARG, b"null"), (dict(llr_in=None), INVALID_ARG, b"null"),
    (dict(skip=None), INVALID_ARG, b"null"), (dict(mcs_bits1=0), INVALID_ARG, b"mcs_bits"),
    (dict(mcs_bits0=9), INVALID_ARG, b"mcs_bits"), (dict(dmrs_symbol_mask=1 << 14), INVALID_ARG, b"dmrs_symbol_mask"),
    (dict(dmrs_symbol_mask=-1), INVALID_ARG, b"dmrs_symbol_mask"),
    (dict(num_symbols=12), SHAPE, b"num_symbols"), (dict(batch=0), SHAPE, b"batch"), (dict(batch=65536), SHAPE, b"batch"),
    (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"), (dict(num_subcarriers=3301), SHAPE, b"num_subcarriers"),
    (dict(num_tx=0), SHAPE, b"num_tx"), (dict(num_tx=17), SHAPE, b"num_tx"), (dict(num_mcs=0), SHAPE, b"num_mcs"),
    (dict(num_mcs=9), SHAPE, b"num_mcs"), (dict(bits_stride=5), SHAPE, b"bits_stride"),
    (dict(num_heads=2), SHAPE, b"num_heads"), (dict(num_cw_per_user=0), SHAPE, b"num_cw_per_user"),
    (dict(num_cw_per_user=65), SHAPE, b"num_cw_per_user"),
    (dict(batch=65535, num_tx=16, num_cw_per_user=2), SHAPE, b"2^20"),
    (dict(n=3), SHAPE, b"n must"), (dict(n=26113), SHAPE, b"n must"), (dict(n_tx=0), SHAPE, b"n_tx"),
    (dict(n_tx=(1 << 20) + 1), SHAPE, b"n_tx"), (dict(tx_col=None, n_tx=129), SHAPE, b"tx_col"),
]


@pytest.mark.parametrize("kw,code,word", GATHER_CASES)
def test_gather_argument_checks(lib, kw, code, word):
    io = _gather_io(**kw)
    assert lib.nrx_ldpc_gather(ctypes.byref(io), None) == code
    assert word in lib.nrx_last_error()


def _count_io(**kw):
    io = _lib.nrx_ldpc_count_io()
    io.batch, io.num_tx, io.num_cw_per_user, io.n, io.num_info = 2, 2, 2, 128, 64
    io.hard = io.skip = io.iters = io.counts = io.iter_counts = 4096
    for k, v in kw.items():
        setattr(io, k, v)
    return io


COUNT_CASES = [
    (dict(hard=None), INVALID_ARG, b"null"), (dict(skip=None), INVALID_ARG, b"null"),
    (dict(counts=None), INVALID_ARG, b"null"), (dict(batch=0), SHAPE, b"batch"), (dict(batch=65536), SHAPE, b"batch"),
    (dict(num_tx=0), SHAPE, b"num_tx"), (dict(num_tx=17), SHAPE, b"num_tx"),
    (dict(num_cw_per_user=0), SHAPE, b"num_cw_per_user"), (dict(num_cw_per_user=65), SHAPE, b"num_cw_per_user"),
    (dict(n=3), SHAPE, b"n must"), (dict(n=26113), SHAPE, b"n must"), (dict(num_info=0), SHAPE, b"num_info"),
    (dict(num_info=129), SHAPE, b"num_info"),
]


@pytest.mark.parametrize("kw,code,word", COUNT_CASES)
def test_count_argument_checks(lib, kw, code, word):
    io = _count_io(**kw)
    assert lib.nrx_ldpc_count(ctypes.byref(io), None) == code
    assert word in lib.nrx_last_error()
    assert lib.nrx_ldpc_gather(None, None) == INVALID_ARG and lib.nrx_ldpc_count(None, None) == INVALID_ARG
