"""The training entry points of include/nrx.h (nrx_train_workspace_size, nrx_train_grad, nrx_adam_step): exports,
the layout of the two new structs and the argument checks, which run before the first HIP call -- so their
status codes are checked here without a GPU."""
import ctypes
import os
import re

import pytest

from neural_rx_amd import _lib
from neural_rx_amd.config import ModelSpec

INVALID_ARG, SHAPE, UNSUPPORTED, WORKSPACE = -1, -2, -3, -6
PTR = 4096          # non-null, 256-byte aligned, never dereferenced on the host
NEW = ("nrx_train_workspace_size", "nrx_train_grad", "nrx_adam_step")
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
    c = _lib.nrx_train_io
    assert ctypes.sizeof(c) == 136
    offsets = {n: getattr(c, n).offset for n, _ in c._fields_}
    assert offsets == dict(shape=0, num_it=16, dmrs_symbol_mask=20, multiloss=24, bits_stride=28, w_chest=32, y=40, pe=48,
                           h_hat=56, active=64, mcs_mask=72, bits=80, h=88, weights=96, grad=104, loss=112, llr=120,
                           h_ref=128)
    c = _lib.nrx_adam_io
    assert ctypes.sizeof(c) == 80
    offsets = {n: getattr(c, n).offset for n, _ in c._fields_}
    assert offsets == dict(n=0, w=8, g=16, m=24, v=32, lr=40, beta1=48, beta2=56, eps=64, step=72)


def test_api_version_and_existing_structs_are_unchanged(lib):
    assert lib.nrx_api_version() == 7
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define NRX_API_VERSION 7\n" in open(os.path.join(root, "include", "nrx.h")).read()
    assert ctypes.sizeof(_lib.nrx_desc) == 80 and ctypes.sizeof(_lib.nrx_shape) == 16 and ctypes.sizeof(_lib.nrx_io) == 80
    assert ctypes.sizeof(_lib.nrx_gen_tc) == 96 and ctypes.sizeof(_lib.nrx_tc_io) == 104
    assert ctypes.sizeof(_lib.nrx_nmse_io) == 72 and ctypes.sizeof(_lib.nrx_count_io) == 104


def _set(s, kw):
    for k, v in kw.items():
        if k in ("batch", "num_tx", "num_subcarriers", "num_symbols"):
            setattr(s.shape, k, v)
        else:
            setattr(s, k, v)
    return s


def _desc(**kw):
    spec = ModelSpec(num_rx_ant=kw.pop("num_rx_ant", 4), d_s=56, num_it=kw.pop("desc_num_it", 2),
                     bits=kw.pop("bits", (4,)), masking=kw.pop("masking", False), use_h_hat=kw.pop("use_h_hat", True))
    d = _lib.make_desc(spec)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _io(**kw):
    io = _lib.nrx_train_io()
    io.shape = _lib.nrx_shape(2, 2, 12, 14)
    io.num_it, io.dmrs_symbol_mask, io.multiloss, io.bits_stride, io.w_chest = 2, (1 << 2) | (1 << 11), 0, 4, 0.02
    io.y = io.pe = io.h_hat = io.active = io.bits = io.h = io.weights = io.grad = io.loss = PTR
    return _set(io, kw)


def _size(lib, d, io):
    n = ctypes.c_size_t(0)
    return lib.nrx_train_workspace_size(ctypes.byref(d) if d is not None else None,
                                        ctypes.byref(io) if io is not None else None, ctypes.byref(n)), n.value


def _grad(lib, d, io, ws=PTR, nbytes=1 << 60):
    return lib.nrx_train_grad(ctypes.byref(d) if d is not None else None, ctypes.byref(io) if io is not None else None,
                              ws, nbytes, None)


IO_CASES = [
    (dict(y=None), INVALID_ARG, b"null"), (dict(pe=None), INVALID_ARG, b"null"), (dict(active=None), INVALID_ARG, b"null"),
    (dict(bits=None), INVALID_ARG, b"null"), (dict(weights=None), INVALID_ARG, b"null"),
    (dict(grad=None), INVALID_ARG, b"null"), (dict(loss=None), INVALID_ARG, b"null"),
    (dict(h_hat=None), INVALID_ARG, b"h_hat"), (dict(h=None), INVALID_ARG, b"h is required"),
    (dict(y=PTR + 2), INVALID_ARG, b"4-byte"), (dict(weights=PTR + 1), INVALID_ARG, b"4-byte"),
    (dict(grad=PTR + 2), INVALID_ARG, b"4-byte"), (dict(h=PTR + 3), INVALID_ARG, b"4-byte"),
    (dict(mcs_mask=PTR + 2), INVALID_ARG, b"4-byte"), (dict(llr=PTR + 2), INVALID_ARG, b"4-byte"),
    (dict(h_ref=PTR + 1), INVALID_ARG, b"4-byte"), (dict(loss=PTR + 4), INVALID_ARG, b"8-byte"),
    (dict(num_symbols=13), SHAPE, b"num_symbols"), (dict(batch=0), SHAPE, b"batch"), (dict(num_tx=17), SHAPE, b"num_tx"),
    (dict(num_subcarriers=0), SHAPE, b"num_subcarriers"),
    (dict(batch=65535, num_tx=16, num_subcarriers=3300), SHAPE, b"2^24"),
    (dict(num_it=0), INVALID_ARG, b"iterations"), (dict(num_it=3), INVALID_ARG, b"iterations"),
    (dict(w_chest=-0.1), INVALID_ARG, b"w_chest"), (dict(w_chest=NAN), INVALID_ARG, b"w_chest"),
    (dict(w_chest=INF), INVALID_ARG, b"w_chest"),
    (dict(multiloss=2), INVALID_ARG, b"multiloss"), (dict(multiloss=-1), INVALID_ARG, b"multiloss"),
    (dict(dmrs_symbol_mask=1 << 14), INVALID_ARG, b"dmrs_symbol_mask"), (dict(dmrs_symbol_mask=-1), INVALID_ARG, b"dmrs_symbol_mask"),
    (dict(dmrs_symbol_mask=(1 << 14) - 1), INVALID_ARG, b"data symbol"),
    (dict(bits_stride=3), SHAPE, b"bits_stride"),
]


@pytest.mark.parametrize("kw,code,word", IO_CASES)
def test_train_argument_checks(lib, kw, code, word):
    d = _desc()
    assert _grad(lib, d, _io(**kw)) == code, kw
    assert word in lib.nrx_last_error()
    assert _size(lib, d, _io(**kw))[0] == code


def test_null_arguments(lib):
    assert _grad(lib, None, _io()) == INVALID_ARG
    assert _grad(lib, _desc(), None) == INVALID_ARG
    assert _grad(lib, _desc(), _io(), ws=None) == INVALID_ARG and b"workspace" in lib.nrx_last_error()
    assert _grad(lib, _desc(), _io(), ws=PTR + 128) == INVALID_ARG and b"256-byte" in lib.nrx_last_error()
    assert lib.nrx_train_workspace_size(ctypes.byref(_desc()), ctypes.byref(_io()), None) == INVALID_ARG
    assert lib.nrx_adam_step(None, None) == INVALID_ARG


def test_what_may_be_null(lib):
    """h with w_chest = 0, h_hat without use_h_hat, mcs_mask, llr and h_ref: every check passes and the call stops
    at the workspace size"""
    for d, io in ((_desc(), _io(w_chest=0.0, h=None)), (_desc(use_h_hat=False), _io(h_hat=None)),
                  (_desc(), _io(llr=PTR, h_ref=PTR, mcs_mask=PTR)), (_desc(), _io(num_it=1, multiloss=1))):
        assert _grad(lib, d, io, nbytes=8) == WORKSPACE


@pytest.mark.parametrize("kw", [dict(d_s=64), dict(agg_units=32), dict(readout_units=64), dict(num_rx_ant=17),
                                dict(num_rx_ant=0), dict(num_it=9), dict(num_mcs=4), dict(num_mcs=9, var_mcs_masking=1)])
def test_topologies_nrx_create_refuses(lib, kw):
    d = _desc(**kw)
    assert _grad(lib, d, _io()) == UNSUPPORTED
    assert _size(lib, d, _io())[0] == UNSUPPORTED
    # the same check, with the same words, as nrx_create
    msg = lib.nrx_last_error()
    h = ctypes.c_void_p()
    assert lib.nrx_create(ctypes.byref(d), None, None, 0, 0, ctypes.byref(h)) == UNSUPPORTED
    assert lib.nrx_last_error() == msg


def test_workspace_one_byte_short(lib):
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for d, io, H, hb, A2, c0 in ((_desc(), _io(), 1, [4], 8, 18),
                                 (_desc(bits=(2, 4)), _io(multiloss=1, batch=3), 2, [2, 4], 8, 18),
                                 (_desc(bits=(2, 4, 6), masking=True, num_rx_ant=3, use_h_hat=False),
                                  _io(num_subcarriers=24, bits_stride=6, h_hat=None, num_it=1), 1, [6], 6, 8)):
        rc, need = _size(lib, d, io)
        assert rc == 0
        # the formula of csrc/nrx_train.hip's header comment
        s = io.shape
        P, it, R = s.batch * s.num_tx * s.num_subcarriers * 14, io.num_it, io.num_it if io.multiloss else 1
        act = lambda c: al(P * c * 4)  # noqa: E731
        want = al(s.batch * 4) + act(c0) + H * (act(c0) + 4 * act(128)) + (it + 1) * act(56)
        want += it * (act(64) + act(56) + 2 * act(114) + 4 * act(128))
        want += R * (sum(act(128) + 2 * act(b) for b in hb) + act(128) + 2 * act(A2))
        want += 2 * act(128) + 2 * act(56) + act(64) + act(56)
        pc = ((P + 255) // 256 + 31) // 32 * 32
        want += al((P + pc - 1) // pc * 129 * 128 * 4) + al(R * H * 256 * 8) + al(R * 256 * 8)
        assert need == want
        assert _grad(lib, d, io, nbytes=need - 1) == WORKSPACE
        assert str(need).encode() in lib.nrx_last_error()


def _adam(**kw):
    io = _lib.nrx_adam_io()
    io.n, io.lr, io.beta1, io.beta2, io.eps, io.step = 100, 1e-3, 0.9, 0.999, 1e-7, 1
    io.w = io.g = io.m = io.v = PTR
    for k, v in kw.items():
        setattr(io, k, v)
    return io


@pytest.mark.parametrize("kw,word", [
    (dict(w=None), b"null"), (dict(g=None), b"null"), (dict(m=None), b"null"), (dict(v=None), b"null"),
    (dict(w=PTR + 2), b"4-byte"), (dict(v=PTR + 1), b"4-byte"), (dict(step=0), b"step"), (dict(step=-3), b"step"),
    (dict(n=-1), b"n must"), (dict(lr=NAN), b"lr"), (dict(lr=-1e-3), b"lr"), (dict(eps=INF), b"eps"),
    (dict(beta1=1.0), b"beta"), (dict(beta2=-0.1), b"beta"), (dict(beta1=NAN), b"beta")])
def test_adam_argument_checks(lib, kw, word):
    assert lib.nrx_adam_step(ctypes.byref(_adam(**kw)), None) == INVALID_ARG
    assert word in lib.nrx_last_error()


def test_save_load_round_trip(tmp_path):
    import numpy as np
    from neural_rx_amd import weights as W
    from neural_rx_amd.receiver import spec_for
    ws = W.seeded(spec_for("nrx_rt"), seed=2)
    path = str(tmp_path / "w.npz")
    W.save(path, ws)
    back = W.load_file(path)
    assert len(back) == len(ws)
    assert all(a.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(back, ws))
    with np.load(path) as d:
        assert int(d["count"]) == len(ws) and "w000" in d and f"w{len(ws) - 1:03d}" in d


def test_train_command_line_refusals(capsys):
    """the refusals shared with the evaluation come before the first import of torch"""
    from neural_rx_amd import train
    for argv, word in ((["-tc_cp", "4"], "give -tc_fft_size"), (["-tc_fft_size", "64", "-cfo_hz", "100"], "one sample-domain stage"),
                       (["-ebno_db_min", "5", "-ebno_db_max", "1"], "-ebno_db_max"), (["-baselines", "lmmse_lmmse"], "unrecognized")):
        with pytest.raises(SystemExit):
            train.main(argv)
        assert word in capsys.readouterr().err, argv
