"""A receive path from time-domain samples (needs an MI355X): one generated batch, its ``y`` modulated per
antenna into I/Q samples, then ``OFDMDemodulator`` -> ``LSEstimator`` -> ``CGNNEngine`` on the samples -- the
snippet of README.md and INTEGRATION.md, executed.

The demodulated grid reproduces ``y`` within the f32 gate of tests/test_gpu_ofdm.py for the round trip,
8 max(floor, 2^-23) with the floor that of the numpy statement run in complex64."""
import numpy as np
import pytest

from tests import ofdm_ref as O

pytestmark = pytest.mark.gpu

B, N = 4, 64


def test_samples_to_llrs():
    import torch
    from neural_rx_amd import weights as W
    from neural_rx_amd.config import get_config
    from neural_rx_amd.generator import GenParams, SlotGenerator
    from neural_rx_amd.ls import DMRSPorts, LSEstimator
    from neural_rx_amd.ofdm import OFDMDemodulator, OFDMModulator, default_cp
    from neural_rx_amd.receiver import CGNNEngine, compute_pe, spec_for

    cfg = get_config("nrx_rt")
    ports = DMRSPorts.for_config(cfg, 2)
    p = GenParams.from_config(cfg, num_prbs=4, dmrs=ports)
    F, A, U = p.num_subcarriers, p.num_rx_ant, p.num_tx
    sb = SlotGenerator(p)(B, 0.02)
    cp = default_cp(N)
    assert F == 48 and cp == 4

    # the transmit side of this test: every antenna's grid as a stream of samples
    samples = OFDMModulator(cp, fft_size=N, layout="cgnn")(sb.y)
    assert samples.shape == (B, A, 14 * (N + cp)) and samples.dtype == torch.complex64

    # the receive side, from the samples on
    demod = OFDMDemodulator(N, 0, cp, num_subcarriers=F, layout="cgnn")
    y = demod(samples)
    est = LSEstimator(ports, F, A, p.dmrs_symbols)
    h_hat = est(y, sb.pilots, sb.active)
    engine = CGNNEngine(spec_for(cfg), W.load(cfg.label))
    pe = torch.from_numpy(compute_pe(U, F, p.dmrs_symbols, p.cdm_group)).cuda()
    llr = engine.forward(y, pe, h_hat, sb.active, num_it=cfg.num_nrx_iter_eval)[0].clone()     # the engine reuses its output
    want = engine.forward(sb.y, pe, sb.h_hat, sb.active, num_it=cfg.num_nrx_iter_eval)[0].clone()
    torch.cuda.synchronize()

    y0 = sb.y.cpu().numpy()
    g = O.from_cgnn(y0)                                       # [B, A, F, T] complex64
    ref = g.astype(np.complex128)
    c64 = O.demodulate(O.modulate(g, N, cp, dtype=np.complex64), N, cp, F, dtype=np.complex64)
    floor = float(np.abs(c64 - ref).max() / np.abs(ref).max())
    err = float(np.abs(O.from_cgnn(y.cpu().numpy()) - ref).max() / np.abs(ref).max())
    print(f"y from samples: err {err:.3g} floor {floor:.3g} gate {8 * max(floor, 2.0 ** -23):.3g}")
    assert err <= 8 * max(floor, 2.0 ** -23)
    assert y.shape == sb.y.shape and h_hat.shape == sb.h_hat.shape
    assert llr.shape == want.shape and tuple(llr.shape[1:]) == (B, U, F, 14, max(p.mcs_bits))
    assert bool(torch.isfinite(llr).all())
    # the same receiver on (nearly) the same inputs decides the same bits nearly everywhere
    agree = float(((llr > 0) == (want > 0)).float().mean())
    print("hard decisions equal to those on the generator's own y:", agree)
    assert agree > 0.99
