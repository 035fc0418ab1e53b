"""Argument checks of the entry points that take an engine handle (nrx_forward, nrx_forward_ex,
nrx_workspace_size_ex and the Aerial contract).  They need a created handle, hence a GPU, but every
case is rejected before any launch: one handle, B = 1, U = 1, F = 12, and each case breaks one rule
of an otherwise complete call (real device buffers, a workspace of the full size)."""
import ctypes

import pytest

from neural_rx_amd import _lib
from neural_rx_amd import weights as W
from neural_rx_amd.config import get_config, spec_from_config

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, SHAPE, WORKSPACE = 0, -1, -2, -6
B, U, F, T = 1, 1, 12, 14
CGNN, SIONNA, SPLIT = 0, 1, 2


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    import torch
    from neural_rx_amd.receiver import CGNNEngine
    cfg = get_config("nrx_rt")
    spec = spec_from_config(cfg)
    assert spec.use_h_hat
    e = Env()
    e.eng = CGNNEngine(spec, W.seeded(spec, seed=5))
    e.lib, e.h, e.spec = e.eng._lib, e.eng._h, spec
    # one zeroed buffer stands for every tensor (the largest, h_hat at F = 18, is a few KB), one for the
    # workspace: a case that slipped through its check would run on valid memory
    e.buf = torch.zeros(1 << 18, dtype=torch.float32, device="cuda:0")
    e.ws = torch.zeros(1 << 24, dtype=torch.uint8, device="cuda:0")
    e.p, e.wsp = e.buf.data_ptr(), e.ws.data_ptr()
    e.stream = torch.cuda.current_stream().cuda_stream
    e.eng.profile(True)
    torch.cuda.synchronize()
    yield e
    # nothing was launched by any rejected call
    torch.cuda.synchronize()
    assert all(n == 0 for n, _ in e.eng.profile_read().values())
    e.eng.close()


def _shape(**kw):
    s = _lib.nrx_shape(B, U, F, T)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _io(e, **kw):
    io = _lib.nrx_io()
    io.shape = _shape()
    io.num_it, io.precision = e.spec.num_it, _lib.NRX_PREC_F16
    io.y = io.pe = io.h_hat = io.active = io.mcs_mask = io.llr = io.h_ref = e.p
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _need(e, precision=_lib.NRX_PREC_F16, layout=None):
    n = ctypes.c_size_t(0)
    s = _shape()
    if layout is None:
        assert e.lib.nrx_workspace_size(e.h, ctypes.byref(s), precision, ctypes.byref(n)) == OK
    else:
        assert e.lib.nrx_workspace_size_ex(e.h, ctypes.byref(s), precision, layout, ctypes.byref(n)) == OK
    assert 0 < n.value <= e.ws.numel()
    return n.value


def _err(e):
    return e.lib.nrx_last_error()


# ---- nrx_forward ----------------------------------------------------------------------------

def test_forward_argument_checks(env):
    e = env
    need = _need(e)
    fwd = lambda io, ws=e.wsp, nbytes=need: e.lib.nrx_forward(e.h, ctypes.byref(io), ws, nbytes, e.stream)
    for num_it in (0, e.spec.num_it + 1, -1):
        assert fwd(_io(e, num_it=num_it)) == INVALID_ARG and b"iterations" in _err(e), num_it
    for t in ("y", "pe", "active", "llr"):
        assert fwd(_io(e, **{t: None})) == INVALID_ARG and b"null" in _err(e), t
    assert fwd(_io(e, h_hat=None)) == INVALID_ARG and b"h_hat" in _err(e)
    for prec in (2, -1):
        assert fwd(_io(e, precision=prec)) == INVALID_ARG and b"precision" in _err(e), prec
    assert fwd(_io(e), ws=None) == WORKSPACE and b"workspace" in _err(e)
    assert fwd(_io(e), nbytes=need - 1) == WORKSPACE
    assert b"workspace too small" in _err(e) and str(need).encode() in _err(e)
    need32 = _need(e, _lib.NRX_PREC_F32X)
    assert fwd(_io(e, precision=_lib.NRX_PREC_F32X), nbytes=need32 - 1) == WORKSPACE and str(need32).encode() in _err(e)
    assert e.lib.nrx_forward(None, ctypes.byref(_io(e)), e.wsp, need, e.stream) == INVALID_ARG
    assert e.lib.nrx_forward(e.h, None, e.wsp, need, e.stream) == INVALID_ARG


SHAPE_CASES = [(dict(num_symbols=12), b"num_symbols"), (dict(batch=0), b"batch"), (dict(batch=65536), b"batch"),
               (dict(num_tx=0), b"num_tx"), (dict(num_tx=17), b"num_tx"), (dict(num_subcarriers=0), b"num_subcarriers"),
               (dict(num_subcarriers=3301), b"num_subcarriers")]


@pytest.mark.parametrize("kw,word", SHAPE_CASES)
def test_shape_checks_of_the_sizing_calls_and_the_forward(env, kw, word):
    e = env
    n = ctypes.c_size_t(0)
    s = _shape(**kw)
    assert e.lib.nrx_workspace_size(e.h, ctypes.byref(s), _lib.NRX_PREC_F16, ctypes.byref(n)) == SHAPE
    assert word in _err(e)
    assert e.lib.nrx_workspace_size_ex(e.h, ctypes.byref(s), _lib.NRX_PREC_F16, SPLIT, ctypes.byref(n)) == SHAPE
    io = _io(e)
    io.shape = s
    assert e.lib.nrx_forward(e.h, ctypes.byref(io), e.wsp, e.ws.numel(), e.stream) == SHAPE and word in _err(e)
    aio = _aerial_io(e)
    aio.shape = s
    assert e.lib.nrx_aerial_workspace_size(e.h, ctypes.byref(aio), ctypes.byref(n)) == SHAPE and word in _err(e)


def test_workspace_size_null_arguments(env):
    e = env
    n = ctypes.c_size_t(0)
    s = _shape()
    assert e.lib.nrx_workspace_size(None, ctypes.byref(s), _lib.NRX_PREC_F16, ctypes.byref(n)) == INVALID_ARG
    assert e.lib.nrx_workspace_size(e.h, None, _lib.NRX_PREC_F16, ctypes.byref(n)) == INVALID_ARG
    assert e.lib.nrx_workspace_size(e.h, ctypes.byref(s), _lib.NRX_PREC_F16, None) == INVALID_ARG
    assert e.lib.nrx_workspace_size(e.h, ctypes.byref(s), 2, ctypes.byref(n)) == INVALID_ARG and b"precision" in _err(e)


# ---- nrx_workspace_size_ex / nrx_forward_ex ------------------------------------------------------

def test_forward_ex_layout_checks(env):
    e = env
    n = ctypes.c_size_t(0)
    s = _shape()
    for layout in (3, -1):
        assert e.lib.nrx_workspace_size_ex(e.h, ctypes.byref(s), _lib.NRX_PREC_F16, layout, ctypes.byref(n)) == INVALID_ARG
        assert b"layout" in _err(e)
        assert e.lib.nrx_forward_ex(e.h, ctypes.byref(_io(e)), layout, None, e.wsp, e.ws.numel(),
                                    e.stream) == INVALID_ARG
        assert b"layout" in _err(e)
    need = _need(e, layout=SPLIT)
    assert need > _need(e) == _need(e, layout=CGNN)
    ex = lambda layout, y_imag, nbytes=need, io=None: e.lib.nrx_forward_ex(
        e.h, ctypes.byref(io or _io(e)), layout, y_imag, e.wsp, nbytes, e.stream)
    assert ex(CGNN, e.p) == INVALID_ARG and b"y_imag" in _err(e)
    assert ex(SPLIT, None) == INVALID_ARG and b"y_imag" in _err(e)
    assert ex(SIONNA, e.p) == INVALID_ARG and b"y_imag" in _err(e)
    assert ex(SPLIT, e.p, io=_io(e, y=None)) == INVALID_ARG
    assert ex(SPLIT, e.p, nbytes=need - 1) == WORKSPACE
    assert b"workspace too small" in _err(e) and str(need).encode() in _err(e)
    assert e.lib.nrx_forward_ex(e.h, ctypes.byref(_io(e)), SPLIT, e.p, None, need, e.stream) == WORKSPACE
    # NRX_Y_CGNN is nrx_forward, with its checks
    assert ex(CGNN, None, io=_io(e, num_it=0)) == INVALID_ARG and b"iterations" in _err(e)
    assert ex(CGNN, None, io=_io(e, pe=None)) == INVALID_ARG and b"null" in _err(e)
    assert e.lib.nrx_forward_ex(None, ctypes.byref(_io(e)), SPLIT, e.p, e.wsp, need, e.stream) == INVALID_ARG
    assert e.lib.nrx_forward_ex(e.h, None, SPLIT, e.p, e.wsp, need, e.stream) == INVALID_ARG


# ---- the Aerial contract -------------------------------------------------------------------------

AERIAL_IN = ("y_real", "y_imag", "h_ls_real", "h_ls_imag", "dmrs_ofdm_pos", "dmrs_subcarrier_pos")


def _aerial_io(e, **kw):
    io = _lib.nrx_aerial_io()
    io.shape = _shape()
    io.num_it, io.precision = e.spec.num_it, _lib.NRX_PREC_F16
    io.num_dmrs_symbols, io.num_dmrs_subcarriers = 2, 6
    for t in AERIAL_IN + ("dmrs_port_mask", "llr", "h_hat"):
        setattr(io, t, e.p)
    for k, v in kw.items():
        if k in ("batch", "num_tx", "num_subcarriers", "num_symbols"):
            setattr(io.shape, k, v)
        else:
            setattr(io, k, v)
    return io


AERIAL_CASES = [
    (dict(num_subcarriers=18), b"num_subcarriers"),
    (dict(num_dmrs_symbols=0), b"num_dmrs_symbols"), (dict(num_dmrs_symbols=15), b"num_dmrs_symbols"),
    (dict(num_dmrs_subcarriers=3), b"num_dmrs_subcarriers"), (dict(num_dmrs_subcarriers=14), b"num_dmrs_subcarriers"),
    (dict(num_dmrs_subcarriers=0), b"num_dmrs_subcarriers"),
]


@pytest.mark.parametrize("kw,word", AERIAL_CASES)
def test_aerial_shape_checks(env, kw, word):
    e = env
    io = _aerial_io(e, **kw)
    n = ctypes.c_size_t(0)
    assert e.lib.nrx_aerial_workspace_size(e.h, ctypes.byref(io), ctypes.byref(n)) == SHAPE and word in _err(e)
    assert e.lib.nrx_forward_aerial(e.h, ctypes.byref(io), e.wsp, e.ws.numel(), e.stream) == SHAPE and word in _err(e)
    assert e.lib.nrx_aerial_preprocess(e.h, ctypes.byref(io), e.p, e.p, e.p, e.p, e.stream) == SHAPE and word in _err(e)


def test_aerial_pointer_and_workspace_checks(env):
    e = env
    n = ctypes.c_size_t(0)
    io = _aerial_io(e)
    assert e.lib.nrx_aerial_workspace_size(e.h, ctypes.byref(io), ctypes.byref(n)) == OK
    need = n.value
    assert _need(e) < need <= e.ws.numel()
    assert e.lib.nrx_aerial_workspace_size(e.h, ctypes.byref(io), None) == INVALID_ARG
    assert e.lib.nrx_aerial_workspace_size(None, ctypes.byref(io), ctypes.byref(n)) == INVALID_ARG
    assert e.lib.nrx_aerial_workspace_size(e.h, None, ctypes.byref(n)) == INVALID_ARG
    bad = _aerial_io(e, precision=2)
    assert e.lib.nrx_aerial_workspace_size(e.h, ctypes.byref(bad), ctypes.byref(n)) == INVALID_ARG
    assert b"precision" in _err(e)
    fwd = lambda io, ws=e.wsp, nbytes=need: e.lib.nrx_forward_aerial(e.h, ctypes.byref(io), ws, nbytes, e.stream)
    for t in AERIAL_IN + ("dmrs_port_mask", "llr"):
        assert fwd(_aerial_io(e, **{t: None})) == INVALID_ARG and b"null" in _err(e), t
    assert fwd(bad) == INVALID_ARG and b"precision" in _err(e)
    assert fwd(io, nbytes=need - 1) == WORKSPACE
    assert b"workspace too small" in _err(e) and str(need).encode() in _err(e)
    assert fwd(io, ws=None) == WORKSPACE and b"workspace" in _err(e)
    assert e.lib.nrx_forward_aerial(None, ctypes.byref(io), e.wsp, need, e.stream) == INVALID_ARG
    assert e.lib.nrx_forward_aerial(e.h, None, e.wsp, need, e.stream) == INVALID_ARG
    pre = lambda io, outs=(e.p,) * 4: e.lib.nrx_aerial_preprocess(e.h, ctypes.byref(io), *outs, e.stream)
    for t in AERIAL_IN:
        assert pre(_aerial_io(e, **{t: None})) == INVALID_ARG and b"null" in _err(e), t
    for k in range(4):
        outs = tuple(None if j == k else e.p for j in range(4))
        assert pre(io, outs) == INVALID_ARG and b"null" in _err(e), k
    assert e.lib.nrx_aerial_preprocess(None, ctypes.byref(io), e.p, e.p, e.p, e.p, e.stream) == INVALID_ARG
    assert e.lib.nrx_aerial_preprocess(e.h, None, e.p, e.p, e.p, e.p, e.stream) == INVALID_ARG
