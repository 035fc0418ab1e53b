"""The time-domain channel's entry points of include/nrx.h (nrx_time_channel, nrx_gen_workspace_size_tc,
nrx_generate_slots_tc): exports, the layout of the two new structs and the argument checks, which run before the
first HIP call -- so their status codes are checked here without a GPU."""
import ctypes
import os
import re

import pytest

from neural_rx_amd import _lib
from neural_rx_amd.generator import GenParams, TimeChannelParams, TimeDomain

INVALID_ARG, SHAPE, WORKSPACE = -1, -2, -6
PTR = 4096          # non-null, 16-byte aligned, never dereferenced on the host
NEW = ("nrx_time_channel", "nrx_gen_workspace_size_tc", "nrx_generate_slots_tc")
NAN, INF = float("nan"), float("inf")
CP = [6] + [4] * 13


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
    c = _lib.nrx_tc_io
    assert ctypes.sizeof(c) == 104
    offsets = {n: getattr(c, n).offset for n, _ in c._fields_}
    assert offsets == dict(batch=0, num_tx=4, num_rx_ant=8, num_paths=12, num_sinusoids=16, l_min=20, l_max=24, pad_=28,
                           num_samples=32, n0=40, sample_rate=48, tau=56, g0=64, fd=72, x=80, rx_mix=88, r=96)
    c = _lib.nrx_gen_tc
    assert ctypes.sizeof(c) == 96
    offsets = {n: getattr(c, n).offset for n, _ in c._fields_}
    assert offsets == dict(fft_size=0, first_bin=4, cp_length=8, l_min=64, l_max=68, timing_advance=72, pad_=76,
                           r_out=80, x_out=88)


def test_api_version_and_existing_structs_are_unchanged(lib):
    assert lib.nrx_api_version() == 7
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define NRX_API_VERSION 7\n" in open(os.path.join(root, "include", "nrx.h")).read()
    assert ctypes.sizeof(_lib.nrx_gen_td) == 160 and ctypes.sizeof(_lib.nrx_ofdm_io) == 200
    assert ctypes.sizeof(_lib.nrx_gen_chan) == 264 and ctypes.sizeof(_lib.nrx_gen_cir) == 56


def _set(s, kw):
    for k, v in kw.items():
        if isinstance(v, dict):
            for i, x in v.items():
                getattr(s, k)[i] = x
        else:
            setattr(s, k, v)
    return s


# ---------------------------------------------------------------- nrx_time_channel

def _io(**kw):
    io = _lib.nrx_tc_io()
    io.batch, io.num_tx, io.num_rx_ant, io.num_paths, io.num_sinusoids = 3, 2, 2, 3, 4
    io.l_min, io.l_max, io.num_samples, io.n0, io.sample_rate = -3, 5, 954, 6, 1.92e6
    io.tau = io.g0 = io.fd = io.x = io.r = PTR
    return _set(io, kw)


IO_CASES = [
    (dict(tau=None), INVALID_ARG, b"null"), (dict(g0=None), INVALID_ARG, b"null"), (dict(fd=None), INVALID_ARG, b"null"),
    (dict(x=None), INVALID_ARG, b"null"), (dict(r=None), INVALID_ARG, b"null"),
    (dict(g0=PTR + 8), INVALID_ARG, b"16-byte"), (dict(x=PTR + 8), INVALID_ARG, b"16-byte"),
    (dict(r=PTR + 8), INVALID_ARG, b"16-byte"), (dict(rx_mix=PTR + 8), INVALID_ARG, b"16-byte"),
    (dict(tau=PTR + 4), INVALID_ARG, b"8-byte"), (dict(fd=PTR + 4), INVALID_ARG, b"8-byte"),
    (dict(sample_rate=0.0), INVALID_ARG, b"sample_rate"), (dict(sample_rate=-1.0), INVALID_ARG, b"sample_rate"),
    (dict(sample_rate=NAN), INVALID_ARG, b"sample_rate"), (dict(sample_rate=INF), INVALID_ARG, b"sample_rate"),
    (dict(batch=0), SHAPE, b"batch"), (dict(batch=65536), SHAPE, b"batch"),
    (dict(num_tx=0), SHAPE, b"num_tx"), (dict(num_tx=17), SHAPE, b"num_tx"),
    (dict(num_rx_ant=0), SHAPE, b"num_rx_ant"), (dict(num_rx_ant=17), SHAPE, b"num_rx_ant"),
    (dict(num_paths=0), SHAPE, b"num_paths"), (dict(num_paths=9), SHAPE, b"num_paths"),
    (dict(num_sinusoids=0), SHAPE, b"num_sinusoids"), (dict(num_sinusoids=17), SHAPE, b"num_sinusoids"),
    (dict(l_min=1), SHAPE, b"l_min"), (dict(l_min=-256), SHAPE, b"l_min"),
    (dict(l_max=-1), SHAPE, b"l_max"), (dict(l_max=256), SHAPE, b"l_max"),
    (dict(l_min=-128, l_max=128), SHAPE, b"span"), (dict(l_min=-255, l_max=1), SHAPE, b"span"),
    (dict(num_samples=0), SHAPE, b"num_samples"), (dict(num_samples=1 << 31), SHAPE, b"num_samples"),
    (dict(n0=1 << 31), SHAPE, b"n0"), (dict(n0=-(1 << 31) - 1), SHAPE, b"n0"),
]


@pytest.mark.parametrize("kw,code,word", IO_CASES)
def test_time_channel_argument_checks(lib, kw, code, word):
    assert lib.nrx_time_channel(ctypes.byref(_io(**kw)), None) == code, kw
    assert word in lib.nrx_last_error()


def test_null_io(lib):
    assert lib.nrx_time_channel(None, None) == INVALID_ARG


def test_every_check_precedes_the_launch(lib):
    """arguments at their limits pass every earlier check and stop at the last one, n0"""
    for kw in (dict(batch=65535, num_tx=16, num_rx_ant=16, num_paths=8, num_sinusoids=16), dict(l_min=-255, l_max=0),
               dict(l_min=0, l_max=255), dict(l_min=-127, l_max=128), dict(l_min=0, l_max=0),
               dict(num_samples=(1 << 31) - 1), dict(num_samples=1), dict(rx_mix=PTR)):
        assert lib.nrx_time_channel(ctypes.byref(_io(n0=1 << 31, **kw)), None) == SHAPE, kw
        assert b"n0" in lib.nrx_last_error(), kw


# ---------------------------------------------------------------- nrx_generate_slots_tc

def _desc(F=48, U=2, A=2, B=3, **kw):
    p = GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A, cdm_group=tuple(u % 2 for u in range(U)), **kw)
    return p.desc(B, 0.01)


def _tc(**kw):
    return _set(TimeChannelParams(fft_size=64, cp=CP).struct(), kw)


def _ref(s):
    return ctypes.byref(s) if s is not None else None


def _generate(lib, d, tc, chan=None, cfo=None, cir=None, td=None, nbytes=1 << 40):
    o = _lib.nrx_gen_out()
    o.y = PTR
    return lib.nrx_generate_slots_tc(ctypes.byref(d), _ref(chan), _ref(cfo), None, _ref(cir), _ref(td), _ref(tc),
                                     ctypes.byref(o), PTR, nbytes, None)


def _size(lib, d, tc, chan=None, cfo=None, cir=None, td=None):
    n = ctypes.c_size_t(0)
    rc = lib.nrx_gen_workspace_size_tc(ctypes.byref(d), _ref(chan), _ref(cfo), None, _ref(cir), _ref(td), _ref(tc),
                                       ctypes.byref(n))
    return rc, n.value


TC_CASES = [
    (dict(fft_size=32), SHAPE, b"fft_size"), (dict(fft_size=100), SHAPE, b"fft_size"), (dict(fft_size=8192), SHAPE, b"fft_size"),
    (dict(first_bin=17), SHAPE, b"first_bin"), (dict(first_bin=-2), SHAPE, b"first_bin"),
    (dict(cp_length={5: 65}), SHAPE, b"cp_length"), (dict(cp_length={0: -1}), SHAPE, b"cp_length"),
    (dict(timing_advance=-1), SHAPE, b"timing_advance"), (dict(timing_advance=5), SHAPE, b"timing_advance"),
    (dict(l_min=1), SHAPE, b"l_min"), (dict(l_min=-256), SHAPE, b"l_min"), (dict(l_max=256), SHAPE, b"l_max"),
    (dict(l_min=-128, l_max=128), SHAPE, b"span"),
    (dict(r_out=PTR + 8), INVALID_ARG, b"r_out"), (dict(x_out=PTR + 8), INVALID_ARG, b"x_out"),
]


@pytest.mark.parametrize("kw,code,word", TC_CASES)
def test_tc_argument_checks(lib, kw, code, word):
    d = _desc()
    assert _generate(lib, d, _tc(**kw)) == code
    assert word in lib.nrx_last_error()
    assert _size(lib, d, _tc(**kw))[0] == code


def test_the_default_l_max_follows_the_longest_port_delay(lib):
    """l_max < 0: ceil(max_delay_s fs) + 6, fs = 64 * 30 kHz; a resolved l_max beyond 255 is refused"""
    assert _size(lib, _desc(max_delay_s=248.5 / 1.92e6), _tc(l_min=0))[0] == 0         # 249 + 6 = 255
    assert _size(lib, _desc(max_delay_s=249.5 / 1.92e6), _tc(l_min=0))[0] == SHAPE and b"l_max" in lib.nrx_last_error()
    assert _size(lib, _desc(max_delay_s=249.5 / 1.92e6), _tc(l_max=9))[0] == 0         # a given l_max is taken
    assert _size(lib, _desc(max_delay_s=244.5 / 1.92e6), _tc(l_min=-6))[0] == SHAPE and b"span" in lib.nrx_last_error()
    chan = _lib.nrx_gen_chan()
    chan.max_delay_s[0], chan.max_delay_s[1], chan.max_delay_s[2] = 1e-7, 300 / 1.92e6, 1.0     # port 2 is not read
    assert _size(lib, _desc(), _tc(), chan=chan)[0] == SHAPE and b"l_max" in lib.nrx_last_error()
    assert _generate(lib, _desc(), _tc(), chan=chan) == SHAPE
    chan.max_delay_s[1] = 2e-7
    assert _size(lib, _desc(), _tc(), chan=chan)[0] == 0


def test_grid_wider_than_the_fft_is_a_shape_error(lib):
    assert _generate(lib, _desc(F=72), _tc()) == SHAPE and b"num_subcarriers" in lib.nrx_last_error()


def test_one_sample_domain_stage_per_call(lib):
    d = _desc()
    cfo = _lib.nrx_gen_cfo()
    assert _generate(lib, d, _tc(), cfo=cfo, nbytes=8) == WORKSPACE        # an all-zero cfo is no cfo
    cfo.cfo_hz[1] = 100.0
    td = TimeDomain(fft_size=64, cp=CP).struct(2)
    cir = _lib.nrx_gen_cir()
    cir.num_examples, cir.num_paths, cir.num_time_steps, cir.select, cir.a, cir.tau = 4, 2, 1, 1, PTR, PTR
    for kw in (dict(cfo=cfo), dict(td=td), dict(cir=cir)):
        assert _generate(lib, d, _tc(), **kw) == INVALID_ARG, kw
        assert b"one sample-domain stage" in lib.nrx_last_error()
        assert _size(lib, d, _tc(), **kw)[0] == INVALID_ARG
        assert _generate(lib, d, None, nbytes=8, **kw) == WORKSPACE        # each of them alone is fine
    for kw in (dict(td=TimeDomain(64)), dict(cfo_hz=100.0)):
        with pytest.raises(ValueError, match="one sample-domain stage"):
            GenParams(num_tx=2, num_subcarriers=48, num_rx_ant=2, tc=TimeChannelParams(64), **kw)


def test_workspace_is_the_generators_plus_the_stage(lib):
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for F, U, A, B, N, cp in ((48, 2, 2, 3, 64, CP), (50, 3, 5, 2, 128, [9] * 14), (24, 1, 1, 1, 4096, [288] * 14)):
        d = _desc(F, U, A, B)
        n = ctypes.c_size_t(0)
        assert lib.nrx_gen_workspace_size(ctypes.byref(d), ctypes.byref(n)) == 0
        base = n.value
        tc = TimeChannelParams(fft_size=N, cp=cp).struct()
        Ls, nsin = sum(cp) + 14 * N, B * U * A * d.num_taps * d.num_sinusoids
        extra = al(B * U * Ls * 16) + al(B * A * Ls * 16) + al(nsin * 16) + al(nsin * 8) + al(B * A * F * 14 * 16)
        assert _size(lib, d, None) == (0, base)
        assert _size(lib, d, tc) == (0, base + extra)
        assert _generate(lib, d, tc, nbytes=base + extra - 1) == WORKSPACE
        assert str(base + extra).encode() in lib.nrx_last_error()
        # tc == NULL is the _td entry point
        m = ctypes.c_size_t(0)
        assert lib.nrx_gen_workspace_size_td(ctypes.byref(d), None, None, None, None, ctypes.byref(m)) == 0
        assert m.value == base
        td = TimeDomain(fft_size=N, cp=cp).struct(U)
        assert lib.nrx_gen_workspace_size_td(ctypes.byref(d), None, None, None, ctypes.byref(td), ctypes.byref(m)) == 0
        assert _size(lib, d, None, td=td) == (0, m.value)


def test_time_channel_params():
    t = TimeChannelParams(4096).struct()
    assert list(t.cp_length) == [288] * 14 and (t.l_min, t.l_max, t.timing_advance, t.first_bin) == (-6, -1, 0, -1)
    p = TimeChannelParams(64, cp=CP, l_min=-2, l_max=9, timing_advance=2, first_bin=3)
    t = p.struct()
    assert (t.l_min, t.l_max, t.timing_advance, t.first_bin) == (-2, 9, 2, 3) and p.num_samples() == 14 * 64 + 58
    with pytest.raises(ValueError):
        TimeChannelParams(64, cp=[4] * 13).struct()


def test_evaluate_flags(capsys):
    """the refusals of the command line, which come before the first import of torch"""
    from neural_rx_amd import evaluate
    for argv, word in ((["-tc_cp", "4"], "give -tc_fft_size"), (["-tc_l_max", "9"], "give -tc_fft_size"),
                       (["-tc_timing_advance", "1"], "give -tc_fft_size"),
                       (["-tc_fft_size", "64", "-td_fft_size", "64"], "one sample-domain stage"),
                       (["-tc_fft_size", "64", "-cfo_hz", "100"], "one sample-domain stage"),
                       (["-max_doppler_hz", "5", "-channel", "double_tdl_low"], "-channel iid"),
                       (["-max_delay_s", "1e-6", "-channel", "double_tdl_high"], "-channel iid")):
        with pytest.raises(SystemExit):
            evaluate.main(argv)
        assert word in capsys.readouterr().err, argv
