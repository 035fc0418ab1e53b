"""nrx_generate_slots_no on the GPU: one noise variance per slot (needs an MI355X).

The property everything rests on: slot ``slot_offset + b`` generated with ``no_slot[b] = x`` is bit for bit the slot a
plain call with ``desc.no = x`` gives at that global index, in every output -- through the grid channel, a replayed
dataset (``cir``) and the time-domain channel (``tc``), each of which has its own noise site.
"""
import ctypes

import numpy as np
import pytest

from tests.memguard import same_bits

pytestmark = pytest.mark.gpu

B, U, F, A = 4, 2, 12, 2
OFF = 5
NO_SLOT = [0.5, 0.05, 0.5, 0.0]
OUTPUTS = ("y", "h_hat", "h", "active", "mcs_mask", "mcs", "bits", "y_real", "y_imag", "h_ls_real", "h_ls_imag")


def _grid_params():
    from neural_rx_amd.generator import GenParams
    return GenParams(num_tx=U, num_subcarriers=F, num_rx_ant=A, cdm_group=(0, 1), mcs_bits=(2, 4), mcs_of_user=(-1, 1),
                     num_active=None, seed=61)


def _cir_params():
    from tests.test_gpu_cir import _channel, _data, _params
    a, tau = _data(2, A, 3, 14)                        # a two-example toy dataset
    return _params(U, F, A, _channel(a, tau, "random", True, "centered"))


def _tc_params():
    import dataclasses
    from neural_rx_amd.generator import TimeChannelParams
    return dataclasses.replace(_grid_params(), num_taps=3, tc=TimeChannelParams(fft_size=64, cp=[6] + [4] * 13))


PATHS = {"grid": _grid_params, "cir": _cir_params, "tc": _tc_params}


def _run(gen, no):
    import torch
    if not isinstance(no, float):
        no = torch.tensor(no, dtype=torch.float64, device="cuda")
    sb = gen(B, no, slot_offset=OFF)
    torch.cuda.synchronize()
    out = {k: getattr(sb, k).cpu().numpy().copy() for k in OUTPUTS}
    assert all(v.shape[0] == B for v in out.values())
    return out


_RUNS = {}


def runs(path):
    """the per-slot call and the plain calls at 0.5, 0.05 and 0 over the same global indices, generated once"""
    if path not in _RUNS:
        from neural_rx_amd.generator import SlotGenerator
        gen = SlotGenerator(PATHS[path](), want_h=True, aerial=True)
        _RUNS[path] = dict(slot=_run(gen, NO_SLOT), **{str(x): _run(gen, x) for x in (0.5, 0.05, 0.0)})
    return _RUNS[path]


@pytest.mark.parametrize("path", list(PATHS))
def test_every_slot_is_the_plain_slot_at_its_own_variance(path):
    r = runs(path)
    for b, x in enumerate(NO_SLOT):
        for k in OUTPUTS:
            assert same_bits(r["slot"][k][b], r[str(x)][k][b]), (path, b, k)
    # ... and the variance matters: the slots at another variance differ in y and in what is estimated from it
    for k in ("y", "h_hat", "y_real", "h_ls_real"):
        assert not same_bits(r["slot"][k][1], r["0.5"][k][1]), k
        assert not same_bits(r["slot"][k][3], r["0.5"][k][3]), k
    assert np.isfinite(r["slot"]["y"]).all() and r["slot"]["active"].any()


class _ThroughNo:
    """``libnrx`` with nrx_generate_slots_tc routed through nrx_generate_slots_no and a fixed noise block"""

    def __init__(self, lib, noise):
        self._lib, self._noise = lib, noise

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def nrx_generate_slots_tc(self, *args):
        return self._lib.nrx_generate_slots_no(*args[:7], self._noise, *args[7:])


@pytest.mark.parametrize("path", list(PATHS))
def test_null_noise_is_generate_slots_tc(path):
    from neural_rx_amd import _lib
    from neural_rx_amd.generator import SlotGenerator
    want = runs(path)["0.05"]
    empty = _lib.nrx_gen_noise()
    assert not empty.no_slot
    for noise in (None, ctypes.byref(empty)):
        gen = SlotGenerator(PATHS[path](), want_h=True, aerial=True)
        gen._lib = _ThroughNo(gen._lib, noise)
        got = _run(gen, 0.05)
        for k in OUTPUTS:
            assert same_bits(got[k], want[k]), (path, k)


def test_noise_variance_ratio():
    """The sample variance of y - (noise-free y) of slot 0 (0.5) over slot 1 (0.05) is 10 within sampling error.
    Each slot has n = 12 * 14 * 2 * 2 = 672 real noise samples of zero mean, so each mean square is
    sigma^2 chi2_n / n with relative standard deviation sqrt(2 / n), and the logarithm of their ratio has the standard
    deviation sqrt(2 / n + 2 / n) = 2 / sqrt(n) = 0.0772: the 4-sigma band is 10 exp(+-0.309) = [7.34, 13.6]."""
    r = runs("grid")
    n = F * 14 * A * 2
    assert n == 672 and r["slot"]["y"][0].size == n
    d = (r["slot"]["y"].astype(np.float64) - r["0.0"]["y"].astype(np.float64)).reshape(B, -1)
    ms = (d * d).mean(axis=1)
    ratio = ms[0] / ms[1]
    sigma_log = 2.0 / np.sqrt(n)
    print(f"mean squares {ms}  ratio {ratio:.3f}  band {10 * np.exp(-4 * sigma_log):.2f}..{10 * np.exp(4 * sigma_log):.2f}")
    assert abs(np.log(ratio / 10.0)) <= 4 * sigma_log
    # the per-component variance itself is no / 2, within the same 4 sigma of one chi-square
    for b in (0, 1):
        assert abs(ms[b] / (NO_SLOT[b] / 2) - 1.0) <= 4 * np.sqrt(2.0 / n)
    assert not d[3].any()                                  # no_slot = 0: no noise at all


def test_wrapper_refuses_a_wrong_tensor():
    import torch
    from neural_rx_amd.generator import SlotGenerator
    gen = SlotGenerator(_grid_params(), want_h=True)
    with pytest.raises(ValueError, match="no must be"):
        gen(B, torch.zeros(B, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="no must be"):
        gen(B, torch.zeros(B + 1, dtype=torch.float64, device="cuda"))
