"""The correlated per-user channel on the GPU (``nrx_generate_slots_ex``, ``nrx_cov_space_accumulate``)
against the numpy statement tests/synth_chan_ref.py (needs an MI355X).

Tolerances: integer outputs (bits, MCS, active ports) bit-exact; float outputs (y, h, h_hat) within
the bound of tests/test_gpu_synth.py (1e-6 relative to max |.| plus 1e-7 absolute: both sides
compute in f64 and round once).  A NULL ``chan`` and a ``chan`` that repeats the desc's scalars
without a mix are bit-identical to ``nrx_generate_slots``; an explicit identity mix only promises
the float bound (its sums add products with zero).

Spatial covariance: every entry within N 2^-52 acc[0][0] of numpy float64 (N = B U F 14 products
per entry: the float64 summation bound); measured max |gpu - ref| / bound on an MI355X: K1 0.006,
K3 0.009, K5 0.007.  Statistical check: 2048 slots of ``double_tdl_high`` (A = 4, alpha = 0.9,
F = 12, seed 7, from slot 2^40) give max |space() - rx_correlation(4, 0.9)| <= 0.01, below the
smallest gap between two different entries of that matrix (1 - 0.9^(1/9) = 0.0116).  The float64
reference tests/synth_chan_ref.py alone gives 0.0029 for the same slots (0.0049 for 1024, 0.0020
for 4096), under half the bound; the GPU gives 0.0029 too.  With alpha = 0 the same count gives
max |space() - I| = 0.020 under a bound of 0.05: an off-diagonal entry of i.i.d. antennas has a
standard deviation of 1 / sqrt(n) for n independent tap draws, n >= 2048 slots x 2 users here, so
0.016 at the most, and 0.05 is three of those.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import synth_ref as S
from tests import synth_chan_ref as C

pytestmark = pytest.mark.gpu

FIELDS = ("y", "h_hat", "h", "active", "mcs_mask", "mcs", "bits")


def _host(sb):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(sb, k).cpu().numpy() for k in FIELDS}


def _gpu(params, batch, no, off=0):
    from neural_rx_amd.generator import SlotGenerator
    return _host(SlotGenerator(params, want_h=True)(batch, no, slot_offset=off))


def _raw(params, batch, no, chan):
    """nrx_generate_slots (chan = "old") or nrx_generate_slots_ex with a given nrx_gen_chan / None"""
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.generator import SlotGenerator
    g = SlotGenerator(params, want_h=True)
    sb = g._alloc(batch)
    d = params.desc(batch, no, 3)
    o = _lib.nrx_gen_out()
    o.y, o.h_hat, o.h, o.active = (t.data_ptr() for t in (sb.y, sb.h_hat, sb.h, sb.active))
    o.mcs_mask, o.mcs, o.bits, o.bits_stride = sb.mcs_mask.data_ptr(), sb.mcs.data_ptr(), sb.bits.data_ptr(), params.bits_max
    ws = torch.empty(g.workspace_bytes(batch), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    if isinstance(chan, str):
        _lib.check(lib.nrx_generate_slots(ctypes.byref(d), ctypes.byref(o), ws.data_ptr(), ws.numel(), st))
    else:
        _lib.check(lib.nrx_generate_slots_ex(ctypes.byref(d), ctypes.byref(chan) if chan is not None else None,
                                             ctypes.byref(o), ws.data_ptr(), ws.numel(), st))
    return _host(sb)


def _close(a, b, name):
    scale = float(np.abs(b).max())
    err = float(np.abs(a.astype(np.float64) - b).max())
    assert err <= 1e-6 * scale + 1e-7, (name, err, scale)


def test_null_and_uniform_chan_are_bit_identical_to_generate_slots():
    import torch
    from neural_rx_amd import _lib
    from neural_rx_amd.generator import GenParams
    p = GenParams(num_tx=2, num_subcarriers=24, num_rx_ant=4, mcs_bits=(2, 4), mcs_of_user=(-1, 0), seed=17)
    B, no = 3, 0.05
    old = _raw(p, B, no, "old")
    null = _raw(p, B, no, None)
    c = _lib.nrx_gen_chan()
    for u in range(2):
        c.max_delay_s[u], c.max_doppler_hz[u] = p.max_delay_s, p.max_doppler_hz
    c.max_delay_s[2] = float("nan")                 # ports >= U are not read
    uni = _raw(p, B, no, c)
    for k in FIELDS:
        assert old[k].tobytes() == null[k].tobytes() == uni[k].tobytes(), k
    eye = torch.zeros((4, 4, 2), dtype=torch.float64, device="cuda")
    eye[:, :, 0] = torch.eye(4, dtype=torch.float64)
    c.rx_mix = eye.data_ptr()
    mix = _raw(p, B, no, c)
    for k in ("active", "mcs", "bits", "mcs_mask"):
        assert np.array_equal(mix[k], old[k]), k
    for k in ("y", "h", "h_hat"):
        _close(mix[k], old[k].astype(np.float64), k)


def _parity(p, B, no, off):
    g = _gpu(p, B, no, off)
    s = S.GenSpec(batch=B, num_tx=p.num_tx, num_subcarriers=p.num_subcarriers, num_rx_ant=p.num_rx_ant,
                  dmrs_symbols=p.dmrs_symbols, cdm_group=p.cdm_group, mcs_bits=p.mcs_bits, mcs_of_user=p.mcs_of_user,
                  num_active=p.num_active, num_taps=p.num_taps, num_sinusoids=p.num_sinusoids,
                  max_delay_s=p.max_delay_s, max_doppler_hz=p.max_doppler_hz, subcarrier_spacing=p.subcarrier_spacing,
                  no=no, seed=p.seed, slot_offset=off)
    o = C.generate(s, p.profiles(), p.rx_mix())
    np.testing.assert_array_equal(g["active"], o.active)
    np.testing.assert_array_equal(g["mcs"], o.mcs)
    np.testing.assert_array_equal(g["bits"], o.bits)
    for k in ("h", "y", "h_hat"):
        _close(g[k], getattr(o, k).astype(np.float64), k)
    return g, o


def test_parity_two_profiles_high_correlation():
    from neural_rx_amd.generator import GenParams, rx_correlation
    p = GenParams(num_tx=2, num_subcarriers=24, num_rx_ant=4, seed=11,
                  user_profiles=[(420e-9, 400.0), (1270e-9, 100.0)], rx_corr=rx_correlation(4, 0.9))
    g, o = _parity(p, 3, 0.05, 5)
    # the two ports do differ from the uniform channel
    q = GenParams(num_tx=2, num_subcarriers=24, num_rx_ant=4, seed=11)
    assert not np.array_equal(_gpu(q, 3, 0.05, 5)["h"], g["h"])


def test_parity_complex_mix_odd_antennas():
    """A = 3 with the square root of a random complex Hermitian PSD matrix: a kernel that used M^T or
    conj(M) would fail here (a real symmetric M cannot tell)"""
    from neural_rx_amd.generator import GenParams
    R = C.random_psd(3, 23)
    p = GenParams(num_tx=3, num_subcarriers=24, num_rx_ant=3, cdm_group=(0, 1, 0), num_active=2, seed=12, rx_corr=R)
    M = p.rx_mix()
    assert np.abs(M.imag).max() > 0.05 and np.abs(M - M.T).max() > 0.05
    g, o = _parity(p, 3, 0.05, 0)
    wrong = C.generate(S.GenSpec(batch=3, num_tx=3, num_subcarriers=24, num_rx_ant=3, cdm_group=(0, 1, 0), num_active=2,
                                 no=0.05, seed=12), p.profiles(), M.T)
    assert np.abs(wrong.h - o.h).max() > 1e-2        # the case can tell M from its transpose


def test_parity_sixteen_antennas_and_a_flat_port():
    from neural_rx_amd.generator import GenParams, rx_correlation
    p = GenParams(num_tx=2, num_subcarriers=12, num_rx_ant=16, seed=13,
                  user_profiles=[(0.0, 30.0), (300e-9, 400.0)], rx_corr=rx_correlation(16, 0.9))
    g, _ = _parity(p, 2, 0.01, 1)
    h0 = g["h"][:, 0]                                # max_delay_s = 0: the same value on every subcarrier
    assert np.abs(h0 - h0[:, :1]).max() <= 1e-6 * np.abs(h0).max()


def test_one_call_equals_two_calls_with_offsets():
    from neural_rx_amd.generator import GenParams, scenario
    p = scenario("double_tdl_high", GenParams(num_tx=2, num_subcarriers=24, num_rx_ant=4, seed=5))
    full = _gpu(p, 4, 0.05, 6)
    for k0 in (0, 2):
        part = _gpu(p, 2, 0.05, 6 + k0)
        for k in FIELDS:
            assert part[k].tobytes() == full[k][k0:k0 + 2].tobytes(), k


# ---- spatial covariance ---------------------------------------------------------------------------

# (U, A, F, B): the K1-, K3- and K5-like shapes of tests/chest_ref.py
COV_CASES = {"K1": (2, 4, 24, 3), "K3": (4, 16, 36, 2), "K5": (2, 1, 12, 2)}


def _cov_params(name):
    from neural_rx_amd.generator import GenParams, rx_correlation
    U, A, F, _ = COV_CASES[name]
    return GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A, cdm_group=tuple(u % 2 for u in range(U)), seed=7,
                     rx_corr=rx_correlation(A, 0.9))


@functools.lru_cache(maxsize=None)
def _cov_slots(name, batch, off=0):
    import torch
    from neural_rx_amd.generator import SlotGenerator
    sb = SlotGenerator(_cov_params(name), want_h=True)(batch, 0.1, slot_offset=off)
    torch.cuda.synchronize()
    h = sb.h.cpu().numpy()
    h.setflags(write=False)
    return sb, h


def _space(name, batches):
    import torch
    from neural_rx_amd.chest import CovarianceEstimator
    cov = CovarianceEstimator(_cov_params(name))
    for sb in batches:
        cov.accumulate(sb)
    torch.cuda.synchronize()
    a = cov.acc_s.cpu().numpy()
    return a[..., 0] + 1j * a[..., 1], cov


@pytest.mark.parametrize("name", list(COV_CASES))
def test_spatial_covariance_sums(name):
    U, A, F, B = COV_CASES[name]
    sb, h = _cov_slots(name, B)
    got, cov = _space(name, [sb])
    ref = C.spatial_sums(h)
    bound = B * U * F * 14 * 2.0 ** -52 * ref[0, 0].real
    ratio = np.abs(got - ref).max() / bound
    print(f"{name}: spatial cov max |gpu - ref| / (N 2^-52 acc[0][0]) = {ratio:.4f}")
    assert ratio <= 1.0, (name, ratio)
    again, _ = _space(name, [sb])
    assert np.array_equal(got.view(np.float64), again.view(np.float64))       # a repeated call: the same bits
    R_s = cov.space()
    assert R_s.shape == (A, A) and np.array_equal(R_s, R_s.conj().T) and np.isclose(np.trace(R_s).real, A)
    R_f, R_t = cov.matrices()                                                  # still the (R_f, R_t) pair
    assert R_f.shape == (F, F) and R_t.shape == (14, 14)


@pytest.mark.parametrize("name", list(COV_CASES))
def test_spatial_covariance_accumulates_over_batches(name):
    import dataclasses
    import torch
    U, A, F, B = COV_CASES[name]
    sb0, _ = _cov_slots(name, B)
    sb1, _ = _cov_slots(name, B, off=B)
    both = dataclasses.replace(sb0, h=torch.cat([sb0.h, sb1.h]).contiguous())
    two, _ = _space(name, [sb0, sb1])
    one, _ = _space(name, [both])
    bound = 2 * B * U * F * 14 * 2.0 ** -52 * one[0, 0].real
    assert np.abs(two - one).max() <= bound


def test_spatial_covariance_approaches_the_correlation_matrix():
    """2048 slots of double_tdl_high, A = 4: max |space() - rx_correlation(4, 0.9)| <= 0.01; the float64
    reference alone gives 0.0029 on the same slots (module docstring)"""
    from neural_rx_amd.chest import estimate_covariance
    from neural_rx_amd.generator import GenParams, SlotGenerator, rx_correlation, scenario
    p = scenario("double_tdl_high", GenParams(num_tx=2, num_subcarriers=12, num_rx_ant=4, seed=7))
    cov = estimate_covariance(SlotGenerator(p, want_h=True), 2048, 256)
    dev = float(np.abs(cov.space() - rx_correlation(4, 0.9)).max())
    print(f"2048 slots: max |R_s - rx_correlation(4, 0.9)| = {dev:.4f}")
    assert dev <= 0.01
    # and an uncorrelated generator gives the identity
    q = scenario("double_tdl_low", GenParams(num_tx=2, num_subcarriers=12, num_rx_ant=4, seed=7))
    low = estimate_covariance(SlotGenerator(q, want_h=True), 2048, 256).space()
    print(f"2048 slots, alpha = 0: max |R_s - I| = {np.abs(low - np.eye(4)).max():.4f}")
    assert np.abs(low - np.eye(4)).max() <= 0.05
