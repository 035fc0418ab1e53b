"""The carrier-frequency-offset entry points of include/nrx.h (nrx_generate_slots_cfo,
nrx_gen_workspace_size_cfo, nrx_cfo_estimate, nrx_cfo_rotate): exports, struct layouts and the argument
checks, which run before the first HIP call -- so their status codes are checked here without a GPU."""
import ctypes
import os
import re

import pytest

from neural_rx_amd import _lib
from neural_rx_amd.generator import GenParams

INVALID_ARG, SHAPE, WORKSPACE = -1, -2, -6
PTR = 4096          # non-null, never dereferenced on the host
NEW = ("nrx_gen_workspace_size_cfo", "nrx_generate_slots_cfo", "nrx_cfo_estimate", "nrx_cfo_rotate")


@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def _desc(F=24, U=2):
    p = GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=2, cdm_group=tuple(u % 2 for u in range(U)))
    return p.desc(3, 0.01)


def _cfo(**kw):
    c = _lib.nrx_gen_cfo()
    c.cfo_hz[0], c.cfo_hz[1] = 100.0, 200.0
    for k, v in kw.items():
        if k.startswith("cfo_hz"):
            c.cfo_hz[int(k[6:])] = v
        else:
            setattr(c, k, v)
    return c


def _out():
    o = _lib.nrx_gen_out()
    o.y = PTR
    return o


def _generate(lib, d, cfo, out=None, ws=PTR, nbytes=1 << 40):
    o = out if out is not None else _out()
    return lib.nrx_generate_slots_cfo(ctypes.byref(d), None, ctypes.byref(cfo) if cfo is not None else None,
                                      ctypes.byref(o), ws, nbytes, None)


def _size(lib, d, cfo):
    n = ctypes.c_size_t(0)
    rc = lib.nrx_gen_workspace_size_cfo(ctypes.byref(d), ctypes.byref(cfo) if cfo is not None else None, ctypes.byref(n))
    return rc, n.value


def test_exports_header_and_layouts(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nrx.h")).read()
    syms = set(re.findall(r"\b(nrx_[a-z_0-9]+)\s*\(", header))
    assert syms == set(_lib.EXPORTS)
    for s in NEW:
        assert s in syms and hasattr(lib, s)
    # nrx_gen_cfo: 16 doubles, 4 int32, one pointer; nrx_cfo_io: 28 int32, 4 pointers
    assert ctypes.sizeof(_lib.nrx_gen_cfo) == 16 * 8 + 4 * 4 + 8 and _lib.nrx_gen_cfo.eps_out.offset == 144
    assert ctypes.sizeof(_lib.nrx_cfo_io) == 28 * 4 + 4 * 8 and _lib.nrx_cfo_io.h_in.offset == 112
    assert _lib.nrx_cfo_io.ref_mode.offset == 104
    # the leading fields are those of nrx_chest_io, in its order
    assert [n for n, _ in _lib.nrx_cfo_io._fields_][:8] == [n for n, _ in _lib.nrx_chest_io._fields_][:8]
    assert f"#define NRX_CFO_REF_NEAREST_DMRS {_lib.CFO_REF_NEAREST_DMRS}\n" in header
    assert f"#define NRX_CFO_REF_ZERO {_lib.CFO_REF_ZERO}\n" in header


def test_api_version_is_unchanged(lib):
    assert lib.nrx_api_version() == 7
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define NRX_API_VERSION 7\n" in open(os.path.join(root, "include", "nrx.h")).read()


GEN_CASES = [
    (dict(cfo_hz0=-1.0), INVALID_ARG, b"carrier frequency offset"),
    (dict(cfo_hz1=float("nan")), INVALID_ARG, b"carrier frequency offset"),
    (dict(cfo_hz1=float("inf")), INVALID_ARG, b"carrier frequency offset"),
    (dict(constant=2), INVALID_ARG, b"constant"), (dict(constant=-1), INVALID_ARG, b"constant"),
    (dict(h_with_phase=2), INVALID_ARG, b"h_with_phase"), (dict(h_with_phase=-1), INVALID_ARG, b"h_with_phase"),
    (dict(eps_out=PTR + 4), INVALID_ARG, b"eps_out"),
    (dict(fft_size=23), SHAPE, b"fft_size"), (dict(fft_size=8193), SHAPE, b"fft_size"),
    (dict(fft_size=-1), SHAPE, b"fft_size"),
]


@pytest.mark.parametrize("kw,code,word", GEN_CASES)
def test_generator_argument_checks(lib, kw, code, word):
    d = _desc()
    assert _generate(lib, d, _cfo(**kw)) == code
    assert word in lib.nrx_last_error()
    assert _size(lib, d, _cfo(**kw))[0] == code


def test_generator_accepts_the_limits_and_ignores_unused_ports(lib):
    d = _desc()
    for kw in (dict(fft_size=24), dict(fft_size=8192), dict(fft_size=0), dict(constant=1, h_with_phase=1),
               dict(cfo_hz2=-5.0), dict(cfo_hz15=float("nan")), dict(eps_out=PTR + 8)):
        assert _size(lib, d, _cfo(**kw))[0] == 0, kw
        # passes every check and stops at the workspace size
        assert _generate(lib, d, _cfo(**kw), nbytes=8) == WORKSPACE, kw


def test_descriptor_and_output_checks_are_those_of_the_generator(lib):
    d = _desc()
    d.num_symbols = 12
    assert _generate(lib, d, _cfo()) == SHAPE
    assert _size(lib, d, _cfo())[0] == SHAPE
    d = _desc()
    d.num_active = 0
    assert _generate(lib, d, _cfo()) == INVALID_ARG
    d = _desc()
    o = _lib.nrx_gen_out()
    assert _generate(lib, d, _cfo(), out=o) == INVALID_ARG and b"null tensor" in lib.nrx_last_error()
    assert lib.nrx_generate_slots_cfo(ctypes.byref(d), None, ctypes.byref(_cfo()), None, PTR, 1 << 40, None) == INVALID_ARG
    assert _generate(lib, d, _cfo(), ws=None) == INVALID_ARG and b"workspace" in lib.nrx_last_error()
    assert lib.nrx_generate_slots_cfo(None, None, None, None, None, 0, None) == INVALID_ARG
    n = ctypes.c_size_t(0)
    assert lib.nrx_gen_workspace_size_cfo(None, None, ctypes.byref(n)) == INVALID_ARG
    assert lib.nrx_gen_workspace_size_cfo(ctypes.byref(d), None, None) == INVALID_ARG
    # a bad per-port channel entry is still reported
    ch = _lib.nrx_gen_chan()
    ch.max_delay_s[1] = -1.0
    assert lib.nrx_generate_slots_cfo(ctypes.byref(d), ctypes.byref(ch), ctypes.byref(_cfo()), ctypes.byref(_out()), PTR,
                                      1 << 40, None) == INVALID_ARG


def test_workspace_is_the_generators_plus_the_offset_grid(lib):
    for F, U in ((24, 2), (2, 2), (133, 3)):
        d = _desc(F, U)
        n = ctypes.c_size_t(0)
        assert lib.nrx_gen_workspace_size(ctypes.byref(d), ctypes.byref(n)) == 0
        base = n.value
        xp = (3 * U * F * 14 * 16 + 255) // 256 * 256
        assert _size(lib, d, None) == (0, base)
        assert _size(lib, d, _cfo(cfo_hz0=0.0, cfo_hz1=0.0)) == (0, base)
        assert _size(lib, d, _cfo(cfo_hz0=0.0, cfo_hz1=0.0, cfo_hz15=9.0)) == (0, base)
        assert _size(lib, d, _cfo()) == (0, base + xp)
        assert _size(lib, d, _cfo(cfo_hz0=0.0)) == (0, base + xp)
        assert _generate(lib, d, _cfo(), nbytes=base + xp - 1) == WORKSPACE
        assert str(base + xp).encode() in lib.nrx_last_error()
        assert _generate(lib, d, _cfo(cfo_hz0=0.0, cfo_hz1=0.0), nbytes=base - 1) == WORKSPACE
        assert str(base).encode() in lib.nrx_last_error()
        assert _generate(lib, d, None, nbytes=base - 1) == WORKSPACE


def _io(**kw):
    io = _lib.nrx_cfo_io()
    io.batch, io.num_tx, io.num_subcarriers, io.num_symbols = 2, 2, 12, 14
    io.num_rx_ant, io.num_dmrs_symbols = 4, 2
    io.dmrs_symbols[0], io.dmrs_symbols[1] = 2, 11
    io.cdm_group[1] = 1
    io.ref_mode, io.sign = _lib.CFO_REF_ZERO, -1
    io.h_in = io.active = io.eps = io.h_out = PTR
    for k, v in kw.items():
        if k.startswith("dmrs_symbols"):
            io.dmrs_symbols[int(k[12:])] = v
        elif k.startswith("cdm_group"):
            io.cdm_group[int(k[9:])] = v
        else:
            setattr(io, k, v)
    return io


BOTH_CASES = [
    (dict(h_in=None), INVALID_ARG, b"null"), (dict(eps=None), INVALID_ARG, b"null"),
    (dict(eps=PTR + 4), INVALID_ARG, b"eps"),
    (dict(dmrs_symbols1=14), INVALID_ARG, b"dmrs_symbols"), (dict(dmrs_symbols1=2), INVALID_ARG, b"dmrs_symbols"),
    (dict(dmrs_symbols0=-1), INVALID_ARG, b"dmrs_symbols"), (dict(cdm_group0=2), INVALID_ARG, b"cdm_group"),
    (dict(num_symbols=12), SHAPE, b"num_symbols"), (dict(batch=0), SHAPE, b"batch"), (dict(batch=65536), SHAPE, b"batch"),
    (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"), (dict(num_subcarriers=3301), SHAPE, b"num_subcarriers"),
    (dict(num_tx=0), SHAPE, b"num_tx"), (dict(num_tx=17), SHAPE, b"num_tx"),
    (dict(num_rx_ant=0), SHAPE, b"num_rx_ant"), (dict(num_rx_ant=17), SHAPE, b"num_rx_ant"),
    (dict(num_dmrs_symbols=0), SHAPE, b"num_dmrs_symbols"), (dict(num_dmrs_symbols=5), SHAPE, b"num_dmrs_symbols"),
]


@pytest.mark.parametrize("kw,code,word", BOTH_CASES)
def test_estimate_and_rotate_argument_checks(lib, kw, code, word):
    io = _io(**kw)
    for fn in (lib.nrx_cfo_estimate, lib.nrx_cfo_rotate):
        assert fn(ctypes.byref(io), None) == code
        assert word in lib.nrx_last_error()


ROTATE_CASES = [
    (dict(h_out=None), b"null"), (dict(ref_mode=2), b"ref_mode"), (dict(ref_mode=-1), b"ref_mode"),
    (dict(sign=0), b"sign"), (dict(sign=2), b"sign"),
]


@pytest.mark.parametrize("kw,word", ROTATE_CASES)
def test_rotate_only_checks(lib, kw, word):
    assert lib.nrx_cfo_rotate(ctypes.byref(_io(**kw)), None) == INVALID_ARG
    assert word in lib.nrx_last_error()


def test_estimate_only_checks_and_null_io(lib):
    assert lib.nrx_cfo_estimate(ctypes.byref(_io(active=None)), None) == INVALID_ARG
    assert b"null" in lib.nrx_last_error()
    assert lib.nrx_cfo_estimate(None, None) == INVALID_ARG
    assert lib.nrx_cfo_rotate(None, None) == INVALID_ARG
