"""The channel-impulse-response entry points of include/nrx.h (nrx_generate_slots_cir,
nrx_gen_workspace_size_cir, nrx_generate_taps): exports, the struct layout and the argument checks, which run
before the first HIP call -- so their status codes are checked here without a GPU."""
import ctypes
import os
import re

import pytest

from neural_rx_amd import _lib
from neural_rx_amd.generator import GenParams

INVALID_ARG, SHAPE, WORKSPACE = -1, -2, -6
PTR = 4096          # non-null, never dereferenced on the host
NEW = ("nrx_gen_workspace_size_cir", "nrx_generate_slots_cir", "nrx_generate_taps")


@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def _desc(F=24, U=2, A=2, B=3):
    p = GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A, cdm_group=tuple(u % 2 for u in range(U)))
    return p.desc(B, 0.01)


def _cir(**kw):
    c = _lib.nrx_gen_cir()
    c.num_examples, c.num_paths, c.num_time_steps, c.select, c.normalize = 7, 40, 14, 1, 1
    c.f_offset = -12.0
    c.a = c.tau = c.index = PTR
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _out():
    o = _lib.nrx_gen_out()
    o.y = PTR
    return o


def _generate(lib, d, cir, chan=None, cfo=None, dmrs=None, out=None, ws=PTR, nbytes=1 << 40):
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
    o = out if out is not None else _out()
    return lib.nrx_generate_slots_cir(ctypes.byref(d), ref(chan), ref(cfo), ref(dmrs), ref(cir), ctypes.byref(o), ws,
                                      nbytes, None)


def _size(lib, d, cir, cfo=None, dmrs=None):
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
    n = ctypes.c_size_t(0)
    return lib.nrx_gen_workspace_size_cir(ctypes.byref(d), ref(cfo), ref(dmrs), ref(cir), ctypes.byref(n)), n.value


def test_exports_header_and_layout(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nrx.h")).read()
    syms = set(re.findall(r"\b(nrx_[a-z_0-9]+)\s*\(", header))
    assert syms == set(_lib.EXPORTS)
    for s in NEW:
        assert s in syms and hasattr(lib, s)
    c = _lib.nrx_gen_cir
    assert ctypes.sizeof(c) == 6 * 4 + 8 + 3 * 8 == 56
    offsets = {n: getattr(c, n).offset for n, _ in c._fields_}
    assert offsets == dict(num_examples=0, num_paths=4, num_time_steps=8, select=12, normalize=16, pad_=20,
                           f_offset=24, a=32, tau=40, index=48)


def test_api_version_and_existing_structs_are_unchanged(lib):
    assert lib.nrx_api_version() == 7
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define NRX_API_VERSION 7\n" in open(os.path.join(root, "include", "nrx.h")).read()
    assert ctypes.sizeof(_lib.nrx_gen_cfo) == 152 and ctypes.sizeof(_lib.nrx_gen_dmrs) == 144
    assert ctypes.sizeof(_lib.nrx_gen_chan) == 264


CASES = [
    (dict(a=None), INVALID_ARG, b"null"), (dict(a=PTR + 4), INVALID_ARG, b"aligned"),
    (dict(tau=None), INVALID_ARG, b"null"),
    (dict(select=0, index=None), INVALID_ARG, b"index"),
    (dict(select=3), INVALID_ARG, b"select"), (dict(select=-1), INVALID_ARG, b"select"),
    (dict(f_offset=float("nan")), INVALID_ARG, b"f_offset"), (dict(f_offset=float("inf")), INVALID_ARG, b"f_offset"),
    (dict(f_offset=float("-inf")), INVALID_ARG, b"f_offset"),
    (dict(num_examples=0), SHAPE, b"num_examples"), (dict(num_examples=(1 << 24) + 1), SHAPE, b"num_examples"),
    (dict(num_paths=0), SHAPE, b"num_paths"), (dict(num_paths=1025), SHAPE, b"num_paths"),
    (dict(num_time_steps=0), SHAPE, b"num_time_steps"), (dict(num_time_steps=2), SHAPE, b"num_time_steps"),
    (dict(num_time_steps=13), SHAPE, b"num_time_steps"),
    (dict(select=2, num_examples=1), SHAPE, b"select 2"),
]


@pytest.mark.parametrize("kw,code,word", CASES)
def test_argument_checks(lib, kw, code, word):
    d = _desc()
    assert _generate(lib, d, _cir(**kw)) == code
    assert word in lib.nrx_last_error()
    assert _size(lib, d, _cir(**kw))[0] == code


def test_a_chan_is_refused_with_a_cir_and_accepted_without(lib):
    d = _desc()
    ch = _lib.nrx_gen_chan()
    assert _generate(lib, d, _cir(), chan=ch) == INVALID_ARG
    assert b"chan" in lib.nrx_last_error()
    assert _generate(lib, d, None, chan=ch, nbytes=8) == WORKSPACE


def test_limits_pass_and_stop_at_the_workspace(lib):
    d = _desc()
    for kw in (dict(num_examples=1), dict(num_examples=1 << 24), dict(num_paths=1), dict(num_paths=1024),
               dict(num_time_steps=1), dict(select=0), dict(select=2, num_examples=2), dict(select=1, index=None),
               dict(select=2, index=None), dict(normalize=0, f_offset=0.0), dict(a=PTR + 8, tau=PTR + 4)):
        assert _size(lib, d, _cir(**kw))[0] == 0, kw
        assert _generate(lib, d, _cir(**kw), nbytes=8) == WORKSPACE, kw


def test_descriptor_and_output_checks_are_those_of_the_generator(lib):
    d = _desc()
    d.num_symbols = 12
    assert _generate(lib, d, _cir()) == SHAPE and _size(lib, d, _cir())[0] == SHAPE
    for field in ("num_taps", "num_sinusoids"):        # validated as always, though a replay does not read them
        d = _desc()
        setattr(d, field, 0)
        assert _generate(lib, d, _cir()) == INVALID_ARG, field
    d = _desc()
    d.max_delay_s = -1.0
    assert _generate(lib, d, _cir()) == INVALID_ARG
    d = _desc()
    assert _generate(lib, d, _cir(), out=_lib.nrx_gen_out()) == INVALID_ARG and b"null tensor" in lib.nrx_last_error()
    assert _generate(lib, d, _cir(), ws=None) == INVALID_ARG and b"workspace" in lib.nrx_last_error()
    assert lib.nrx_generate_slots_cir(None, None, None, None, None, None, None, 0, None) == INVALID_ARG
    n = ctypes.c_size_t(0)
    assert lib.nrx_gen_workspace_size_cir(None, None, None, None, ctypes.byref(n)) == INVALID_ARG
    assert lib.nrx_gen_workspace_size_cir(ctypes.byref(d), None, None, ctypes.byref(_cir()), None) == INVALID_ARG
    cfo = _lib.nrx_gen_cfo()
    cfo.cfo_hz[0] = -1.0
    assert _generate(lib, d, _cir(), cfo=cfo) == INVALID_ARG


def test_workspace_is_the_generators_plus_the_replayed_channel(lib):
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for F, U, A, B in ((24, 2, 2, 3), (50, 3, 5, 2), (133, 1, 16, 1)):
        d = _desc(F, U, A, B)
        n = ctypes.c_size_t(0)
        assert lib.nrx_gen_workspace_size(ctypes.byref(d), ctypes.byref(n)) == 0
        base = n.value
        tiles, groups = (F + 63) // 64, ((14 * A + 15) // 16 * 16 + 63) // 64
        extra = al(B * U * F * 14 * A * 16) + al(B * U * tiles * groups * 8) + al(B * U * 8)
        assert _size(lib, d, None) == (0, base)
        assert _size(lib, d, _cir()) == (0, base + extra)
        assert _size(lib, d, _cir(num_paths=1024, num_time_steps=1)) == (0, base + extra)   # no function of L
        assert _generate(lib, d, _cir(), nbytes=base + extra - 1) == WORKSPACE
        assert str(base + extra).encode() in lib.nrx_last_error()
        assert _generate(lib, d, None, nbytes=base - 1) == WORKSPACE
        cfo = _lib.nrx_gen_cfo()
        cfo.cfo_hz[0] = 100.0
        assert _size(lib, d, _cir(), cfo=cfo) == (0, base + al(B * U * F * 14 * 16) + extra)
        # cir == NULL is the _dmrs entry point
        m = ctypes.c_size_t(0)
        assert lib.nrx_gen_workspace_size_dmrs(ctypes.byref(d), ctypes.byref(cfo), None, ctypes.byref(m)) == 0
        assert _size(lib, d, None, cfo=cfo) == (0, m.value)


def test_generate_taps_checks(lib):
    d = _desc()
    call = lambda d, chan=None, a=PTR, tau=PTR, ws=PTR, nbytes=1 << 40: lib.nrx_generate_taps(  # noqa: E731
        ctypes.byref(d) if d is not None else None, ctypes.byref(chan) if chan is not None else None, a, tau, ws, nbytes,
        None)
    assert call(None) == INVALID_ARG
    assert call(d, a=None) == INVALID_ARG and b"null" in lib.nrx_last_error()
    assert call(d, tau=None) == INVALID_ARG
    assert call(d, ws=None) == INVALID_ARG and b"workspace" in lib.nrx_last_error()
    n = ctypes.c_size_t(0)
    assert lib.nrx_gen_workspace_size(ctypes.byref(d), ctypes.byref(n)) == 0
    assert call(d, nbytes=n.value - 1) == WORKSPACE and str(n.value).encode() in lib.nrx_last_error()
    ch = _lib.nrx_gen_chan()
    ch.max_doppler_hz[1] = float("nan")
    assert call(d, chan=ch) == INVALID_ARG
    ch = _lib.nrx_gen_chan()
    ch.rx_mix = PTR + 4
    assert call(d, chan=ch) == INVALID_ARG and b"rx_mix" in lib.nrx_last_error()
    bad = _desc()
    bad.num_taps = 9
    assert call(bad) == INVALID_ARG
