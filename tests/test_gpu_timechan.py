"""``nrx_time_channel`` on the GPU against the numpy statement tests/timechan_ref.py (needs an MI355X).

Tolerance, the project's floor pattern: ``e_ref`` is the largest error of the float64 numpy statement against the
same statement in ``np.longdouble`` on the same inputs, and the kernel, measured against the longdouble result
too, has to stay within ``8 max(e_ref, 1e-15 max|r|)``.  Both figures are printed (DESIGN.md section 9 holds the
table).  An error above the gate is a finding about the rotations or the order of accumulation, not a reason to
widen it.

Shapes.  B = 3, U = 2, L = 3, NS = 4, fs = 64 * 30 kHz, Doppler up to +-20 kHz and +-400 Hz.  A = 2 runs the kernel with a tile of
1024 samples and 3 recurrence steps, A = 5 with 512 and 1, A = 9 with 256 and none; Ls = 954 (one slot at N = 64:
less than one tile), 2500 (no multiple of any tile, several workgroups per row) and 256 (exactly one tile of the
widest kernel); spans (0, 0), (-3, 5), (-6, 40) and 256 taps.  The output is the NaN-poisoned body of a guarded
buffer (tests/memguard.py): every element written, nothing beyond.

EDGES (below) adds the ends of every loop and table of the kernel, at both Doppler ranges and under the same gate:
A = 4, 8, 16 and 1, NS = 16 and 1, L = 1 and 8, U = 1.  Figures of an MI355X run (e_ref from numpy, the kernel's
error against the longdouble statement, the gate), at 20 kHz with rx_mix / at 400 Hz without:

    A   NS  L  U  Ls    taps     e_ref     kernel    gate     |  e_ref     kernel    gate
    4   16  1  1  954   -3..5    4.56e-14  1.60e-14  3.65e-13 |  3.54e-15  2.66e-15  5.13e-14
    8   16  3  2  954   -3..5    5.84e-14  3.36e-14  4.67e-13 |  5.99e-15  4.99e-15  1.07e-13
    16  16  8  2  256   -6..40   5.36e-14  2.10e-14  4.29e-13 |  3.26e-14  9.17e-15  2.61e-13
    1   1   8  2  2500  -3..5    5.15e-13  3.64e-13  4.12e-12 |  7.87e-15  7.80e-15  1.62e-13
"""
import functools

import numpy as np
import pytest

from tests import memguard
from tests import timechan_ref as R

pytestmark = pytest.mark.gpu

B, U, L, NS = 3, 2, 3, 4
FS = 64 * 30e3
N0 = 6

# (A, Ls, l_min, l_max, rx_mix, max delay in samples, max Doppler in Hz).  At 20 kHz the phases reach tens of cycles
# and e_ref, the float64 rounding of the statement's own phase, sets the gate; at 400 Hz the floor 1e-15 max|r| does,
# and the kernel's own roundings (table product, recurrence, sums) are what is measured.
CASES = [
    (2, 954, 0, 0, False, 0.4, 20e3), (2, 954, -3, 5, False, 3.0, 20e3), (2, 954, -3, 5, True, 3.0, 20e3),
    (2, 954, -6, 40, True, 30.0, 20e3), (2, 2500, -100, 155, False, 120.0, 20e3), (2, 2500, -3, 5, True, 3.0, 20e3),
    (5, 2500, -3, 5, True, 3.0, 20e3), (5, 954, -6, 40, False, 30.0, 20e3),
    (9, 954, -3, 5, True, 3.0, 20e3), (9, 256, -6, 40, False, 30.0, 20e3),
    (2, 2500, -3, 5, True, 3.0, 400.0), (5, 954, -6, 40, False, 30.0, 400.0), (9, 954, -3, 5, False, 3.0, 400.0),
]


# (A, NS, L, U, Ls, l_min, l_max, max delay in samples), each at both Doppler ranges: the edges of the kernel's
# shapes.  A = 4, 8, 16 fill k_timechan<4, 4>, <8, 2>, <16, 1> to their last accumulator and make the last chunk of
# four antennas a full one (A = 16: all four chunks); NS = 16 fills the 64 rows of the sinusoid tables of a chunk,
# NS = 1 leaves one row per antenna; L = 1 and 8 and U = 1 are the ends of the path and user loops; A = 1 is one
# antenna in a chunk of four.  rx_mix is on at 20 kHz and off at 400 Hz.
EDGES = [
    (4, 16, 1, 1, 954, -3, 5, 3.0),
    (8, 16, 3, 2, 954, -3, 5, 3.0),
    (16, 16, 8, 2, 256, -6, 40, 30.0),
    (1, 1, 8, 2, 2500, -3, 5, 3.0),
]


@functools.lru_cache(maxsize=None)
def _inputs(A, Ls, dmax, fmax=20e3, seed=11, U=U, L=L, NS=NS):
    rng = np.random.default_rng(seed + 131 * A + Ls)
    cn = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)  # noqa: E731
    x = cn(B, U, Ls)
    tau = rng.uniform(0.0, dmax / FS, (B, U, L))
    g0 = cn(B, U, A, L, NS) / np.sqrt(2 * NS)
    fd = rng.uniform(-fmax, fmax, (B, U, A, L, NS))
    mix = cn(A, A) / np.sqrt(A)
    return x, tau, g0, fd, mix


@functools.lru_cache(maxsize=None)
def _reference(A, Ls, l_min, l_max, mixed, dmax, fmax, U=U, L=L, NS=NS):
    """(longdouble result, e_ref): computed once per case, shared and left unchanged"""
    x, tau, g0, fd, mix = _inputs(A, Ls, dmax, fmax, U=U, L=L, NS=NS)
    m = mix if mixed else None
    r64 = R.time_channel(x, tau, g0, fd, FS, N0, l_min, l_max, m)
    rld = R.time_channel(x, tau, g0, fd, FS, N0, l_min, l_max, m, real=np.longdouble)
    return rld, float(np.abs(r64 - rld).max())


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(x, tau, g0, fd, mix, l_min, l_max, n0=N0):
    import torch
    from neural_rx_amd.timechannel import TimeChannel
    chan = TimeChannel(FS, l_min, l_max, n0)
    out, guard = memguard.guarded_out((x.shape[0], g0.shape[2], x.shape[2]), 0xFF, torch.complex128)
    got = chan(_dev(x), _dev(tau), _dev(g0), _dev(fd), None if mix is None else _dev(mix), out=out)
    torch.cuda.synchronize()
    guard.check("r")
    return got.cpu().numpy()


@pytest.mark.parametrize("A,Ls,l_min,l_max,mixed,dmax,fmax", CASES)
def test_against_the_statement(A, Ls, l_min, l_max, mixed, dmax, fmax):
    _gate_check(A, Ls, l_min, l_max, mixed, dmax, fmax)


def _gate_check(A, Ls, l_min, l_max, mixed, dmax, fmax, **shape):
    x, tau, g0, fd, mix = _inputs(A, Ls, dmax, fmax, **shape)
    rld, e_ref = _reference(A, Ls, l_min, l_max, mixed, dmax, fmax, **shape)
    got = _run(x, tau, g0, fd, mix if mixed else None, l_min, l_max)
    assert got.shape == rld.shape
    assert np.isfinite(got.view(np.float64)).all()                       # every element written
    scale = float(np.abs(rld).max())
    err = float(np.abs(got - rld).max())
    gate = 8.0 * max(e_ref, 1e-15 * scale)
    tag = "".join(f" {k}={v}" for k, v in shape.items())
    print(f"A={A}{tag} Ls={Ls} taps {l_min}..{l_max} mix={mixed} fd<={fmax:g}: e_ref {e_ref:.3g} kernel {err:.3g} "
          f"gate {gate:.3g} max|r| {scale:.3g}")
    assert err <= gate


@pytest.mark.parametrize("fmax", [20e3, 400.0])
@pytest.mark.parametrize("A,NS,L,U,Ls,l_min,l_max,dmax", EDGES)
def test_edges_of_the_kernel_shapes(A, NS, L, U, Ls, l_min, l_max, dmax, fmax):
    _gate_check(A, Ls, l_min, l_max, fmax == 20e3, dmax, fmax, U=U, L=L, NS=NS)


def test_an_integer_delay_without_doppler_shifts_and_scales():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 1, 700)) + 1j * rng.standard_normal((2, 1, 700))
    g0 = rng.standard_normal((2, 1, 3, 1, 1)) + 1j * rng.standard_normal((2, 1, 3, 1, 1))
    fd = np.zeros(g0.shape)
    for k in (0, 1, 5):
        tau = np.full((2, 1, 1), k / FS)
        got = _run(x, tau, g0, fd, None, -3, 5, n0=17)
        want = np.zeros((2, 3, 700), np.complex128)
        want[:, :, k:] = g0[:, 0, :, 0, 0, None] * x[:, 0, None, :700 - k]
        rld = R.time_channel(x, tau, g0, fd, FS, 17, -3, 5, real=np.longdouble)
        e_ref = float(np.abs(R.time_channel(x, tau, g0, fd, FS, 17, -3, 5) - rld).max())
        err, scale = float(np.abs(got - rld).max()), float(np.abs(want).max())
        print(f"delay {k}: e_ref {e_ref:.3g} kernel {err:.3g} against the shift {np.abs(got - want).max():.3g}")
        assert err <= 8.0 * max(e_ref, 1e-15 * scale)
        assert np.abs(got - want).max() <= 1e-13 * scale


@pytest.mark.parametrize("A,Ls,l_min,l_max", [(2, 2500, -3, 5), (5, 954, -6, 40), (9, 954, -3, 5)])
def test_repeat_calls_and_batch_splits_give_the_same_bits(A, Ls, l_min, l_max):
    x, tau, g0, fd, mix = _inputs(A, Ls, 3.0)
    full = _run(x, tau, g0, fd, mix, l_min, l_max)
    assert memguard.same_bits(_run(x, tau, g0, fd, mix, l_min, l_max), full)
    first = _run(x[:2], tau[:2], g0[:2], fd[:2], mix, l_min, l_max)
    second = _run(x[2:], tau[2:], g0[2:], fd[2:], mix, l_min, l_max)
    assert memguard.same_bits(first, full[:2]) and memguard.same_bits(second, full[2:])


def test_the_wrapper_checks_its_tensors():
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.timechannel import TimeChannel
    x, tau, g0, fd, mix = (_dev(v) for v in _inputs(2, 954, 3.0))
    chan = TimeChannel(FS, -3, 5, N0)
    with pytest.raises(ValueError, match="tau must be"):
        chan(x, tau[:, :, :2].contiguous(), g0, fd)
    with pytest.raises(ValueError, match="x must be"):
        chan(x.to(torch.complex64), tau, g0, fd)
    with pytest.raises(ValueError, match="on the GPU"):
        chan(x.cpu(), tau, g0, fd)
    with pytest.raises(_lib.NRXError) as e:
        TimeChannel(FS, -200, 200, N0)(x, tau, g0, fd)
    assert e.value.code == -2 and "span" in str(e.value)
    torch.cuda.synchronize()
