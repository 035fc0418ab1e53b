"""nrx_train_grad_acc and nrx_generate_slots_no (include/nrx.h): exports, the layout of the two new structs and the
argument checks, which all run before the first HIP call -- so their status codes are checked here without a GPU,
in the way of tests/test_train_abi.py and tests/test_tc_abi.py."""
import ctypes

import pytest

from neural_rx_amd import _lib
from tests.test_train_abi import INVALID_ARG, IO_CASES, PTR, SHAPE, UNSUPPORTED, WORKSPACE, _desc, _io

OK = 0


@pytest.fixture(scope="module")
def lib():
    from neural_rx_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_exports_and_layout(lib):
    for s in ("nrx_train_grad_acc", "nrx_generate_slots_no"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    c = _lib.nrx_train_acc
    assert ctypes.sizeof(c) == 8
    assert {n: getattr(c, n).offset for n, _ in c._fields_} == dict(accumulate=0, batch_total=4)
    c = _lib.nrx_gen_noise
    assert ctypes.sizeof(c) == 8 and c.no_slot.offset == 0
    assert lib.nrx_api_version() == 7
    # the structs the new calls take are the old ones
    assert ctypes.sizeof(_lib.nrx_train_io) == 136 and ctypes.sizeof(_lib.nrx_gen_tc) == 96


def _acc(lib, d, io, acc, ws=PTR, nbytes=8):
    """the call with a workspace of 8 bytes: a call that passes every check stops at NRX_ERR_WORKSPACE"""
    return lib.nrx_train_grad_acc(ctypes.byref(d) if d is not None else None,
                                  ctypes.byref(io) if io is not None else None,
                                  ctypes.byref(acc) if acc is not None else None, ws, nbytes, None)


@pytest.mark.parametrize("accumulate,total,code,word", [
    (2, 2, INVALID_ARG, b"accumulate"), (-1, 2, INVALID_ARG, b"accumulate"),
    (0, 1, SHAPE, b"batch_total"), (1, 1, SHAPE, b"batch_total"), (1, 0, SHAPE, b"batch_total"),
    (1, -5, SHAPE, b"batch_total"), (0, 65536, SHAPE, b"batch_total"), (1, 1 << 30, SHAPE, b"batch_total"),
])
def test_acc_refusals(lib, accumulate, total, code, word):
    assert _acc(lib, _desc(), _io(), _lib.nrx_train_acc(accumulate, total)) == code
    assert word in lib.nrx_last_error()


@pytest.mark.parametrize("accumulate,total", [(0, 2), (1, 2), (0, 3), (1, 65535)])
def test_acc_accepted(lib, accumulate, total):
    """shape.batch <= batch_total <= 65535 with accumulate 0 / 1: every check passes, the 8-byte workspace is refused"""
    assert _acc(lib, _desc(), _io(), _lib.nrx_train_acc(accumulate, total)) == WORKSPACE
    assert _acc(lib, _desc(), _io(), None) == WORKSPACE             # acc == NULL: nrx_train_grad


@pytest.mark.parametrize("kw,code,word", IO_CASES)
def test_acc_checks_the_io_as_train_grad_does(lib, kw, code, word):
    for acc in (None, _lib.nrx_train_acc(1, 8)):
        assert _acc(lib, _desc(), _io(**kw), acc, nbytes=1 << 60) == code, kw
        assert word in lib.nrx_last_error()


def test_acc_null_and_workspace(lib):
    acc = _lib.nrx_train_acc(1, 4)
    assert _acc(lib, None, _io(), acc) == INVALID_ARG
    assert _acc(lib, _desc(), None, acc) == INVALID_ARG
    assert _acc(lib, _desc(), _io(), acc, ws=None, nbytes=1 << 60) == INVALID_ARG and b"workspace" in lib.nrx_last_error()
    assert _acc(lib, _desc(), _io(), acc, ws=PTR + 128, nbytes=1 << 60) == INVALID_ARG
    assert _acc(lib, _desc(d_s=64), _io(), acc) == UNSUPPORTED
    # the io is checked before the acc, the acc before the workspace
    assert _acc(lib, _desc(), _io(batch=0), _lib.nrx_train_acc(2, 0)) == SHAPE and b"batch" in lib.nrx_last_error()
    assert _acc(lib, _desc(), _io(), _lib.nrx_train_acc(2, 4), ws=None) == INVALID_ARG
    assert b"accumulate" in lib.nrx_last_error()
    # the workspace is that of nrx_train_workspace_size for the call's own shape, whatever batch_total
    n = ctypes.c_size_t()
    assert lib.nrx_train_workspace_size(ctypes.byref(_desc()), ctypes.byref(_io()), ctypes.byref(n)) == OK
    assert _acc(lib, _desc(), _io(), _lib.nrx_train_acc(1, 128), nbytes=n.value - 1) == WORKSPACE
    assert str(n.value).encode() in lib.nrx_last_error()


# ---------------------------------------------------------------- nrx_generate_slots_no
def _gen_desc(**kw):
    from neural_rx_amd.generator import GenParams
    d = GenParams(num_tx=2, num_subcarriers=12, num_rx_ant=2).desc(4, 0.1)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _gen_out(**kw):
    o = _lib.nrx_gen_out()
    o.y = o.h_hat = o.active = o.mcs_mask = o.mcs = o.bits = PTR
    o.bits_stride = 4
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _gen_no(lib, d, noise, out, ws=PTR, nbytes=8, tc=None):
    r = ctypes.byref
    return lib.nrx_generate_slots_no(r(d) if d is not None else None, None, None, None, None, None,
                                     r(tc) if tc is not None else None, r(noise) if noise is not None else None,
                                     r(out) if out is not None else None, ws, nbytes, None)


def _noise(p):
    n = _lib.nrx_gen_noise()
    n.no_slot = p
    return n


def test_no_slot_alignment(lib):
    for p in (PTR + 1, PTR + 2, PTR + 4, PTR + 7):
        assert _gen_no(lib, _gen_desc(), _noise(p), _gen_out()) == INVALID_ARG
        assert b"no_slot" in lib.nrx_last_error() and b"8-byte" in lib.nrx_last_error()


def test_no_slot_accepted(lib):
    """NULL noise, a NULL no_slot and an aligned one pass every check and stop at the 8-byte workspace"""
    for n in (None, _noise(None), _noise(PTR), _noise(PTR + 8)):
        assert _gen_no(lib, _gen_desc(), n, _gen_out()) == WORKSPACE
    # the size asked for is that of nrx_gen_workspace_size_tc
    need = ctypes.c_size_t()
    assert lib.nrx_gen_workspace_size_tc(ctypes.byref(_gen_desc()), None, None, None, None, None, None,
                                         ctypes.byref(need)) == OK
    assert _gen_no(lib, _gen_desc(), _noise(PTR), _gen_out(), nbytes=need.value - 1) == WORKSPACE
    assert str(need.value).encode() in lib.nrx_last_error()


def test_no_checks_are_those_of_generate_slots_tc(lib):
    n = _noise(PTR)
    assert _gen_no(lib, None, n, _gen_out()) == INVALID_ARG
    assert _gen_no(lib, _gen_desc(), n, None) == INVALID_ARG
    assert _gen_no(lib, _gen_desc(), n, _gen_out(y=None)) == INVALID_ARG
    assert _gen_no(lib, _gen_desc(batch=0), n, _gen_out()) == SHAPE
    assert _gen_no(lib, _gen_desc(no=-1.0), n, _gen_out()) == INVALID_ARG
    assert _gen_no(lib, _gen_desc(), n, _gen_out(bits_stride=1)) == SHAPE
    assert _gen_no(lib, _gen_desc(), n, _gen_out(y_real=PTR)) == INVALID_ARG and b"pairs" in lib.nrx_last_error()
    tc = _lib.nrx_gen_tc()
    tc.fft_size, tc.first_bin, tc.l_min, tc.l_max = 63, -1, -6, 20
    assert _gen_no(lib, _gen_desc(), n, _gen_out(), tc=tc) == SHAPE
    # the descriptor is checked before the noise block
    assert _gen_no(lib, _gen_desc(batch=0), _noise(PTR + 4), _gen_out()) == SHAPE
    assert _gen_no(lib, _gen_desc(), _noise(PTR + 4), _gen_out(y=None)) == INVALID_ARG and b"no_slot" in lib.nrx_last_error()
    assert _gen_no(lib, _gen_desc(), n, _gen_out(), ws=None, nbytes=1 << 60) == INVALID_ARG
