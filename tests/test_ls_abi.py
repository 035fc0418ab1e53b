"""The cover-coded DMRS entry points of include/nrx.h (nrx_ls_estimate, nrx_generate_slots_dmrs,
nrx_gen_workspace_size_dmrs): exports, struct layouts and the argument checks, which run before the
first HIP call -- so their status codes are checked here without a GPU."""
import ctypes
import os
import re

import pytest

from neural_rx_amd import _lib
from neural_rx_amd.generator import GenParams

INVALID_ARG, SHAPE, WORKSPACE = -1, -2, -6
PTR = 4096          # non-null, never dereferenced on the host
NEW = ("nrx_ls_estimate", "nrx_gen_workspace_size_dmrs", "nrx_generate_slots_dmrs")
ARRAYS = ("dmrs_symbols", "cdm_group", "focc", "tocc")


@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def _set(s, kw):
    for k, v in kw.items():
        for a in ARRAYS:
            if k.startswith(a) and k[len(a):].isdigit():
                getattr(s, a)[int(k[len(a):])] = v
                break
        else:
            setattr(s, k, v)
    return s


def _io(**kw):
    """8 ports on 24 subcarriers, DMRS symbols 2 3 10 11, every output asked for"""
    io = _lib.nrx_ls_io()
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = 2, 8, 24, 14
    io.num_rx_ant, io.num_dmrs_symbols = 4, 4
    for k, t in enumerate((2, 3, 10, 11)):
        io.dmrs_symbols[k] = t
    for u in range(8):
        io.cdm_group[u], io.focc[u], io.tocc[u] = (u >> 1) & 1, u & 1, (u >> 2) & 1
    io.despread_f = io.despread_t = 1
    io.y = io.pilots = io.active = io.h_hat = io.h_ls_real = io.h_ls_imag = PTR
    return _set(io, kw)


def test_exports_header_and_layouts(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nrx.h")).read()
    syms = set(re.findall(r"\b(nrx_[a-z_0-9]+)\s*\(", header))
    assert syms == set(_lib.EXPORTS)
    for s in NEW:
        assert s in syms and hasattr(lib, s)
    # nrx_ls_io: 60 int32 (6 scalars, dmrs_symbols[4], three [16] arrays, 2 flags), 6 pointers
    assert ctypes.sizeof(_lib.nrx_ls_io) == 60 * 4 + 6 * 8 and _lib.nrx_ls_io.y.offset == 240
    assert _lib.nrx_ls_io.focc.offset == 104 and _lib.nrx_ls_io.despread_f.offset == 232
    # the leading fields are those of nrx_chest_io, in its order
    assert [n for n, _ in _lib.nrx_ls_io._fields_][:8] == [n for n, _ in _lib.nrx_chest_io._fields_][:8]
    # nrx_gen_dmrs: 34 int32, one pointer
    assert ctypes.sizeof(_lib.nrx_gen_dmrs) == 34 * 4 + 8 and _lib.nrx_gen_dmrs.pilots_out.offset == 136
    assert lib.nrx_api_version() == 7


LS_CASES = [
    (dict(y=None), INVALID_ARG, b"null"), (dict(pilots=None), INVALID_ARG, b"null"),
    (dict(h_hat=None, h_ls_real=None, h_ls_imag=None), INVALID_ARG, b"null output"),
    (dict(h_ls_imag=None), INVALID_ARG, b"pairs"), (dict(h_ls_real=None), INVALID_ARG, b"pairs"),
    (dict(focc3=2), INVALID_ARG, b"focc"), (dict(focc0=-1), INVALID_ARG, b"focc"),
    (dict(tocc7=2), INVALID_ARG, b"tocc"), (dict(tocc1=-1), INVALID_ARG, b"tocc"),
    (dict(despread_f=2), INVALID_ARG, b"despread_f"), (dict(despread_f=-1), INVALID_ARG, b"despread_f"),
    (dict(despread_t=2), INVALID_ARG, b"despread_t"), (dict(despread_t=-1), INVALID_ARG, b"despread_t"),
    (dict(focc1=0), INVALID_ARG, b"share"),                                  # port 1 becomes port 0
    (dict(cdm_group4=1, tocc4=0), INVALID_ARG, b"share"),                    # port 4 becomes port 2
    (dict(tocc6=0), INVALID_ARG, b"share"),                                  # port 6 becomes port 2
    (dict(despread_f=0), INVALID_ARG, b"needs despread_f"),
    (dict(despread_t=0), INVALID_ARG, b"needs despread_t"),
    (dict(num_subcarriers=22, h_ls_real=None, h_ls_imag=None), SHAPE, b"% 4"),
    (dict(num_subcarriers=18, h_ls_real=None, h_ls_imag=None), SHAPE, b"% 4"),
    (dict(num_subcarriers=20), SHAPE, b"% 12"),                              # the Aerial list
    (dict(num_dmrs_symbols=3), INVALID_ARG, b"pairs"),                       # odd
    (dict(dmrs_symbols1=4, dmrs_symbols2=10), INVALID_ARG, b"pairs"),        # 2 4 10 11: not adjacent
    (dict(dmrs_symbols2=9), INVALID_ARG, b"pairs"),                          # 2 3 9 11
    (dict(dmrs_symbols1=14), INVALID_ARG, b"dmrs_symbols"), (dict(dmrs_symbols1=2), INVALID_ARG, b"dmrs_symbols"),
    (dict(cdm_group0=2), INVALID_ARG, b"cdm_group"),
    (dict(num_symbols=12), SHAPE, b"num_symbols"), (dict(batch=0), SHAPE, b"batch"),
    (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"), (dict(num_subcarriers=3304), SHAPE, b"num_subcarriers"),
    (dict(num_tx=0), SHAPE, b"num_tx"), (dict(num_tx=17), SHAPE, b"num_tx"),
    (dict(num_rx_ant=0), SHAPE, b"num_rx_ant"), (dict(num_rx_ant=17), SHAPE, b"num_rx_ant"),
    (dict(num_dmrs_symbols=0), SHAPE, b"num_dmrs_symbols"), (dict(num_dmrs_symbols=5), SHAPE, b"num_dmrs_symbols"),
]


@pytest.mark.parametrize("kw,code,word", LS_CASES)
def test_ls_estimate_argument_checks(lib, kw, code, word):
    assert lib.nrx_ls_estimate(ctypes.byref(_io(**kw)), None) == code
    assert word in lib.nrx_last_error()


def test_ls_estimate_null_io(lib):
    assert lib.nrx_ls_estimate(None, None) == INVALID_ARG
    assert b"NULL" in lib.nrx_last_error()


def _desc(F=24, U=8, dmrs=(2, 3, 10, 11)):
    p = GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=2, dmrs_symbols=dmrs,
                  cdm_group=tuple((u >> 1) & 1 for u in range(U)))
    return p.desc(3, 0.01)


def _dmrs(U=8, **kw):
    m = _lib.nrx_gen_dmrs()
    for u in range(U):
        m.focc[u], m.tocc[u] = u & 1, (u >> 2) & 1
    m.despread_f, m.despread_t = 1, int(U > 4)
    return _set(m, kw)


def _out(**kw):
    o = _lib.nrx_gen_out()
    o.y = PTR
    return _set(o, kw)


def _generate(lib, d, dmrs, out=None, ws=PTR, nbytes=1 << 40):
    o = out if out is not None else _out()
    return lib.nrx_generate_slots_dmrs(ctypes.byref(d), None, None, ctypes.byref(dmrs) if dmrs is not None else None,
                                       ctypes.byref(o), ws, nbytes, None)


def _size(lib, d, dmrs):
    n = ctypes.c_size_t(0)
    rc = lib.nrx_gen_workspace_size_dmrs(ctypes.byref(d), None, ctypes.byref(dmrs) if dmrs is not None else None,
                                         ctypes.byref(n))
    return rc, n.value


GEN_CASES = [
    (dict(focc3=2), INVALID_ARG, b"focc"), (dict(tocc0=-1), INVALID_ARG, b"tocc"),
    (dict(despread_f=2), INVALID_ARG, b"despread_f"), (dict(despread_t=-1), INVALID_ARG, b"despread_t"),
    (dict(focc1=0), INVALID_ARG, b"share"), (dict(despread_f=0), INVALID_ARG, b"needs despread_f"),
    (dict(despread_t=0), INVALID_ARG, b"needs despread_t"),
]


@pytest.mark.parametrize("kw,code,word", GEN_CASES)
def test_generator_argument_checks(lib, kw, code, word):
    d = _desc()
    assert _generate(lib, d, _dmrs(**kw)) == code
    assert word in lib.nrx_last_error()
    assert _size(lib, d, _dmrs(**kw))[0] == code


def test_generator_grid_rules(lib):
    assert _generate(lib, _desc(F=22), _dmrs()) == SHAPE and b"% 4" in lib.nrx_last_error()
    assert _generate(lib, _desc(dmrs=(2, 11)), _dmrs()) == INVALID_ARG and b"pairs" in lib.nrx_last_error()
    assert _generate(lib, _desc(dmrs=(2, 3, 9, 11)), _dmrs()) == INVALID_ARG and b"pairs" in lib.nrx_last_error()
    assert _generate(lib, _desc(dmrs=(2, 3, 10)), _dmrs()) == INVALID_ARG and b"pairs" in lib.nrx_last_error()
    o = _out(h_ls_real=PTR, h_ls_imag=PTR)
    assert _generate(lib, _desc(F=20), _dmrs(), out=o) == SHAPE and b"% 12" in lib.nrx_last_error()
    # the descriptor and output checks are the generator's
    d = _desc()
    d.num_active = 0
    assert _generate(lib, d, _dmrs()) == INVALID_ARG
    assert _generate(lib, _desc(), _dmrs(), out=_lib.nrx_gen_out()) == INVALID_ARG and b"null tensor" in lib.nrx_last_error()
    assert _generate(lib, _desc(), _dmrs(), ws=None) == INVALID_ARG and b"workspace" in lib.nrx_last_error()
    assert lib.nrx_generate_slots_dmrs(None, None, None, None, None, None, 0, None) == INVALID_ARG


def test_ports_beyond_num_tx_are_not_read(lib):
    # the port checks are one function for both entry points; the generator stops at the workspace size,
    # so a call that passes every check launches nothing here
    d = _desc(U=4, dmrs=(2, 11))
    m = _dmrs(U=4)
    for u in range(4, 16):
        m.focc[u], m.tocc[u] = -3, 99
        d.cdm_group[u] = 7
    assert _size(lib, d, m)[0] == 0
    assert _generate(lib, d, m, nbytes=8) == WORKSPACE
    # ... and a bad entry below num_tx is read
    m.focc[3] = 5
    assert _generate(lib, d, m, nbytes=8) == INVALID_ARG


def test_workspace_is_the_generators_plus_the_pilot_table(lib):
    for F, U, dmrs in ((24, 8, (2, 3, 10, 11)), (24, 4, (2, 11)), (132, 2, (2,))):
        d = _desc(F, U, dmrs)
        n = ctypes.c_size_t(0)
        assert lib.nrx_gen_workspace_size(ctypes.byref(d), ctypes.byref(n)) == 0
        base = n.value
        tab = (2 * ((F + 1) // 2) * len(dmrs) * 2 * 4 + 255) // 256 * 256
        assert _size(lib, d, None) == (0, base)
        assert _size(lib, d, _dmrs(U)) == (0, base + tab)
        assert _generate(lib, d, _dmrs(U), nbytes=base + tab - 1) == WORKSPACE
        assert str(base + tab).encode() in lib.nrx_last_error()
        assert _generate(lib, d, None, nbytes=base - 1) == WORKSPACE and str(base).encode() in lib.nrx_last_error()
        assert lib.nrx_gen_workspace_size_dmrs(ctypes.byref(d), None, None, None) == INVALID_ARG
