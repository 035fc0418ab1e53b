"""The OFDM entry points of include/nrx.h (nrx_ofdm_modulate, nrx_ofdm_demodulate, nrx_gen_workspace_size_td,
nrx_generate_slots_td): exports, the layout of the two new structs and the argument checks, which run before
the first HIP call -- so their status codes are checked here without a GPU."""
import ctypes
import os
import re

import pytest

from neural_rx_amd import _lib
from neural_rx_amd.generator import GenParams, TimeDomain

INVALID_ARG, SHAPE, WORKSPACE = -1, -2, -6
PTR = 4096          # non-null, 16-byte aligned, never dereferenced on the host
NEW = ("nrx_ofdm_modulate", "nrx_ofdm_demodulate", "nrx_gen_workspace_size_td", "nrx_generate_slots_td")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_exports_header_and_layout(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nrx.h")).read()
    syms = set(re.findall(r"\b(nrx_[a-z_0-9]+)\s*\(", header))
    assert syms == set(_lib.EXPORTS)
    for s in NEW:
        assert s in syms and hasattr(lib, s)
    c = _lib.nrx_ofdm_io
    assert ctypes.sizeof(c) == 200
    offsets = {n: getattr(c, n).offset for n, _ in c._fields_}
    assert offsets == dict(batch=0, num_streams=4, grid_subcarriers=8, num_symbols=12, fft_size=16, first_bin=20,
                           cp_length=24, precision=80, grid_layout=84, timing_advance=88, offset=92, num_samples=160,
                           pa_asat=168, pa_smoothness=176, grid=184, samples=192)
    c = _lib.nrx_gen_td
    assert ctypes.sizeof(c) == 160
    offsets = {n: getattr(c, n).offset for n, _ in c._fields_}
    assert offsets == dict(fft_size=0, first_bin=4, cp_length=8, delay=64, pa_enable=128, h_with_delay=132,
                           pa_ibo_db=136, pa_smoothness=144, x_out=152)
    for name, val in (("NRX_OFDM_F32", 0), ("NRX_OFDM_F64", 1), ("NRX_OFDM_GRID_PLANAR", 0), ("NRX_OFDM_GRID_CGNN", 1)):
        assert re.search(rf"#define {name}\s+{val}\b", header)


def test_api_version_and_existing_structs_are_unchanged(lib):
    assert lib.nrx_api_version() == 7
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define NRX_API_VERSION 7\n" in open(os.path.join(root, "include", "nrx.h")).read()
    assert ctypes.sizeof(_lib.nrx_gen_cfo) == 152 and ctypes.sizeof(_lib.nrx_gen_dmrs) == 144
    assert ctypes.sizeof(_lib.nrx_gen_chan) == 264 and ctypes.sizeof(_lib.nrx_gen_cir) == 56


# ---------------------------------------------------------------- nrx_ofdm_modulate / nrx_ofdm_demodulate

def _io(**kw):
    io = _lib.nrx_ofdm_io()
    io.batch, io.num_streams, io.grid_subcarriers, io.num_symbols = 2, 3, 48, 14
    io.fft_size, io.first_bin = 64, -1
    for t in range(14):
        io.cp_length[t] = 6 if t == 0 else 4
    io.precision, io.grid_layout, io.timing_advance = 0, 0, 0
    io.num_samples = 14 * 64 + 6 + 13 * 4
    io.grid = io.samples = PTR
    for k, v in kw.items():
        if isinstance(v, dict):
            for i, x in v.items():
                getattr(io, k)[i] = x
        else:
            setattr(io, k, v)
    return io


L0 = 14 * 64 + 6 + 13 * 4
BOTH = [
    (dict(grid=None), INVALID_ARG, b"null"), (dict(samples=None), INVALID_ARG, b"null"),
    (dict(precision=2), INVALID_ARG, b"precision"), (dict(precision=-1), INVALID_ARG, b"precision"),
    (dict(grid_layout=2), INVALID_ARG, b"grid_layout"), (dict(grid_layout=-1), INVALID_ARG, b"grid_layout"),
    (dict(samples=PTR + 4), INVALID_ARG, b"samples"), (dict(grid=PTR + 4), INVALID_ARG, b"grid"),
    (dict(precision=1, samples=PTR + 8), INVALID_ARG, b"samples"), (dict(precision=1, grid=PTR + 8), INVALID_ARG, b"grid"),
    (dict(grid_layout=1, grid=PTR + 2), INVALID_ARG, b"grid"),
    (dict(grid_layout=1, precision=1, grid=PTR + 4), INVALID_ARG, b"grid"),
    (dict(fft_size=32), SHAPE, b"fft_size"), (dict(fft_size=96), SHAPE, b"fft_size"),
    (dict(fft_size=8192, num_samples=1 << 20), SHAPE, b"fft_size"), (dict(fft_size=0), SHAPE, b"fft_size"),
    (dict(grid_subcarriers=65), SHAPE, b"grid_subcarriers"), (dict(grid_subcarriers=0), SHAPE, b"grid_subcarriers"),
    (dict(first_bin=17), SHAPE, b"first_bin"), (dict(first_bin=-2), SHAPE, b"first_bin"),
    (dict(cp_length={3: 65}), SHAPE, b"cp_length"), (dict(cp_length={13: -1}), SHAPE, b"cp_length"),
    (dict(num_samples=L0 - 1), SHAPE, b"num_samples"),
    (dict(batch=0), SHAPE, b"batch"), (dict(batch=65536), SHAPE, b"batch"),
    (dict(num_streams=0), SHAPE, b"num_streams"), (dict(num_streams=17), SHAPE, b"num_streams"),
    (dict(num_symbols=0), SHAPE, b"num_symbols"), (dict(num_symbols=15), SHAPE, b"num_symbols"),
]


@pytest.mark.parametrize("kw,code,word", BOTH)
def test_argument_checks_of_both_calls(lib, kw, code, word):
    for fn in (lib.nrx_ofdm_modulate, lib.nrx_ofdm_demodulate):
        assert fn(ctypes.byref(_io(**kw)), None) == code, kw
        assert word in lib.nrx_last_error()


def test_null_io(lib):
    assert lib.nrx_ofdm_modulate(None, None) == INVALID_ARG and lib.nrx_ofdm_demodulate(None, None) == INVALID_ARG


def test_checks_of_one_call_only(lib):
    """the amplifier is the modulator's, the timing advance the demodulator's: the other call does not read them"""
    for p in (0.0, -1.0, NAN, INF):
        assert lib.nrx_ofdm_modulate(ctypes.byref(_io(pa_asat=1.0, pa_smoothness=p)), None) == INVALID_ARG, p
        assert b"pa_smoothness" in lib.nrx_last_error()
        io = _io(pa_asat=1.0, pa_smoothness=p, num_samples=L0 - 1)      # one sample short: the last check
        assert lib.nrx_ofdm_demodulate(ctypes.byref(io), None) == SHAPE and b"num_samples" in lib.nrx_last_error()
        io = _io(pa_asat=0.0, pa_smoothness=p, num_samples=L0 - 1)      # a linear amplifier reads no smoothness
        assert lib.nrx_ofdm_modulate(ctypes.byref(io), None) == SHAPE and b"num_samples" in lib.nrx_last_error()
    for ta in (-1, 5):                                          # min cp_length is 4
        assert lib.nrx_ofdm_demodulate(ctypes.byref(_io(timing_advance=ta)), None) == SHAPE, ta
        assert b"timing_advance" in lib.nrx_last_error()
    io = _io(timing_advance=99, num_samples=L0 - 1)
    assert lib.nrx_ofdm_modulate(ctypes.byref(io), None) == SHAPE and b"num_samples" in lib.nrx_last_error()
    # T = 1 reads only cp_length[0] = 6
    assert lib.nrx_ofdm_demodulate(ctypes.byref(_io(num_symbols=1, timing_advance=6, num_samples=69)), None) == SHAPE
    assert b"num_samples" in lib.nrx_last_error()
    assert lib.nrx_ofdm_demodulate(ctypes.byref(_io(num_symbols=1, timing_advance=7)), None) == SHAPE


def test_every_check_precedes_the_launch(lib):
    """arguments at their limits pass every shape check and stop at a later one (a misaligned pointer last is
    not possible: alignment is checked early; so the probe is num_samples one short)"""
    for kw in (dict(fft_size=4096, grid_subcarriers=4096, first_bin=0), dict(fft_size=4096, grid_subcarriers=1,
               first_bin=4095), dict(batch=65535, num_streams=16), dict(num_symbols=1),
               dict(cp_length={t: 64 for t in range(14)}), dict(cp_length={t: 0 for t in range(14)}),
               dict(precision=1, grid_layout=1, grid=PTR + 8), dict(grid_layout=1, grid=PTR + 4)):
        io = _io(**kw)
        io.num_samples = sum(io.cp_length[t] + io.fft_size for t in range(io.num_symbols)) - 1
        for fn in (lib.nrx_ofdm_modulate, lib.nrx_ofdm_demodulate):
            assert fn(ctypes.byref(io), None) == SHAPE, kw
            assert b"num_samples" in lib.nrx_last_error(), kw


# ---------------------------------------------------------------- nrx_generate_slots_td

def _desc(F=48, U=2, A=2, B=3):
    p = GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A, cdm_group=tuple(u % 2 for u in range(U)))
    return p.desc(B, 0.01)


def _td(**kw):
    t = TimeDomain(fft_size=64, cp=[6] + [4] * 13, delay=(0, 3)).struct(2)
    for k, v in kw.items():
        if isinstance(v, dict):
            for i, x in v.items():
                getattr(t, k)[i] = x
        else:
            setattr(t, k, v)
    return t


def _ref(s):
    return ctypes.byref(s) if s is not None else None


def _generate(lib, d, td, cfo=None, nbytes=1 << 40):
    o = _lib.nrx_gen_out()
    o.y = PTR
    return lib.nrx_generate_slots_td(ctypes.byref(d), None, _ref(cfo), None, None, _ref(td), ctypes.byref(o), PTR, nbytes,
                                     None)


def _size(lib, d, td, cfo=None):
    n = ctypes.c_size_t(0)
    return lib.nrx_gen_workspace_size_td(ctypes.byref(d), _ref(cfo), None, None, _ref(td), ctypes.byref(n)), n.value


TD_CASES = [
    (dict(delay={1: -1}), INVALID_ARG, b"delay"),
    (dict(pa_enable=2), INVALID_ARG, b"pa_enable"), (dict(h_with_delay=-1), INVALID_ARG, b"h_with_delay"),
    (dict(pa_enable=1, pa_ibo_db=NAN), INVALID_ARG, b"pa_ibo_db"), (dict(pa_enable=1, pa_ibo_db=INF), INVALID_ARG, b"pa_ibo_db"),
    (dict(pa_enable=1, pa_smoothness=0.0), INVALID_ARG, b"pa_smoothness"),
    (dict(pa_enable=1, pa_smoothness=NAN), INVALID_ARG, b"pa_smoothness"),
    (dict(x_out=PTR + 4), INVALID_ARG, b"x_out"),
    (dict(fft_size=32), SHAPE, b"fft_size"), (dict(fft_size=100), SHAPE, b"fft_size"), (dict(fft_size=8192), SHAPE, b"fft_size"),
    (dict(first_bin=17), SHAPE, b"first_bin"), (dict(first_bin=-2), SHAPE, b"first_bin"),
    (dict(cp_length={5: 65}), SHAPE, b"cp_length"), (dict(cp_length={0: -1}), SHAPE, b"cp_length"),
]


@pytest.mark.parametrize("kw,code,word", TD_CASES)
def test_td_argument_checks(lib, kw, code, word):
    d = _desc()
    assert _generate(lib, d, _td(**kw)) == code
    assert word in lib.nrx_last_error()
    assert _size(lib, d, _td(**kw))[0] == code


def test_td_grid_wider_than_the_fft_is_a_shape_error(lib):
    assert _generate(lib, _desc(F=72), _td()) == SHAPE and b"num_subcarriers" in lib.nrx_last_error()


def test_td_and_cfo_exclude_each_other(lib):
    d = _desc()
    cfo = _lib.nrx_gen_cfo()
    assert _generate(lib, d, _td(), cfo=cfo, nbytes=8) == WORKSPACE        # an all-zero cfo is no cfo
    cfo.cfo_hz[1] = 100.0
    assert _generate(lib, d, _td(), cfo=cfo) == INVALID_ARG and b"one transmit-side stage" in lib.nrx_last_error()
    assert _size(lib, d, _td(), cfo=cfo)[0] == INVALID_ARG
    with pytest.raises(ValueError):
        GenParams(num_tx=2, num_subcarriers=48, num_rx_ant=2, cfo_hz=100.0, td=TimeDomain(64))


def test_unread_fields_are_not_checked(lib):
    """the amplifier's parameters without pa_enable, entries of ports >= U"""
    d = _desc()
    for kw in (dict(pa_ibo_db=NAN, pa_smoothness=-1.0), dict(delay={2: -5})):
        assert _size(lib, d, _td(**kw))[0] == 0, kw
        assert _generate(lib, d, _td(**kw), nbytes=8) == WORKSPACE, kw


def test_workspace_is_the_generators_plus_the_grid_and_the_samples(lib):
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for F, U, A, B, N, cp in ((48, 2, 2, 3, 64, [6] + [4] * 13), (50, 3, 5, 2, 128, [9] * 14), (24, 1, 1, 1, 4096, [288] * 14)):
        d = _desc(F, U, A, B)
        n = ctypes.c_size_t(0)
        assert lib.nrx_gen_workspace_size(ctypes.byref(d), ctypes.byref(n)) == 0
        base = n.value
        td = TimeDomain(fft_size=N, cp=cp).struct(U)
        extra = al(B * U * F * 14 * 16) + al(B * U * (sum(cp) + 14 * N) * 16)
        assert _size(lib, d, None) == (0, base)
        assert _size(lib, d, td) == (0, base + extra)
        o = _lib.nrx_gen_out()
        o.y = PTR
        call = lambda td, nbytes: lib.nrx_generate_slots_td(ctypes.byref(d), None, None, None, None, _ref(td),  # noqa: E731
                                                            ctypes.byref(o), PTR, nbytes, None)
        assert call(td, base + extra - 1) == WORKSPACE and str(base + extra).encode() in lib.nrx_last_error()
        assert call(None, base - 1) == WORKSPACE and str(base).encode() in lib.nrx_last_error()
        # td == NULL is the _cir entry point
        m = ctypes.c_size_t(0)
        assert lib.nrx_gen_workspace_size_cir(ctypes.byref(d), None, None, None, ctypes.byref(m)) == 0 and m.value == base


def test_time_domain_params():
    t = TimeDomain(4096, delay=5).struct(3)
    assert list(t.cp_length) == [288] * 14 and list(t.delay)[:4] == [5, 5, 5, 0] and t.first_bin == -1
    assert t.pa_enable == 0 and t.h_with_delay == 0
    t = TimeDomain(64, cp=4, delay=(0, 7), pa_ibo_db=3.0, pa_smoothness=3.0, h_with_delay=True).struct(2)
    assert (t.pa_enable, t.h_with_delay, t.pa_ibo_db, t.pa_smoothness) == (1, 1, 3.0, 3.0)
    with pytest.raises(ValueError):
        TimeDomain(64, delay=(1, 2, 3)).struct(2)
    with pytest.raises(ValueError):
        TimeDomain(64, cp=[4] * 13).struct(2)
