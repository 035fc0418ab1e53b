"""The stage combinations a generator call admits (nrx_api.cpp plan_gen), as ``GenParams``, for the tests of
the generator's workspace: tests/test_workspace_sizes.py (its size) and tests/test_gpu_generator_memory.py
(what a call reads and writes of it).

One sample-domain stage per call (cfo, td or tc), a replayed channel (cir) with a cfo or a td but not with a
tc or per-port profiles, cover-coded pilots (dmrs) with anything.
"""
import numpy as np

from neural_rx_amd.cir import CIRChannel, CIRDataset
from neural_rx_amd.generator import GenParams, TimeChannelParams, TimeDomain, rx_correlation
from neural_rx_amd.ls import DMRSPorts

# name -> stages: chan (per-port profiles and rx_mix), cfo, dmrs, cir1 / cir14 (time steps), td, tc
COMBOS = {
    "none": (), "chan": ("chan",), "cfo": ("cfo",), "dmrs": ("dmrs",), "cfo_dmrs": ("cfo", "dmrs"),
    "cir1": ("cir1",), "cir14": ("cir14",), "cir_dmrs_cfo": ("cir14", "dmrs", "cfo"),
    "td": ("td",), "td_dmrs": ("td", "dmrs"), "td_cir": ("td", "cir1"),
    "tc": ("tc",), "tc_dmrs": ("tc", "dmrs"), "tc_chan": ("tc", "chan"),
}
# cp None: the numerology's own prefixes (ofdm.default_cp)
SHAPES = {
    "tiny": dict(batch=3, num_tx=2, num_subcarriers=24, num_rx_ant=2, num_taps=2, fft_size=64, cp=[6] + [4] * 13),
    "full": dict(batch=128, num_tx=8, num_subcarriers=3276, num_rx_ant=16, num_taps=6, fft_size=4096, cp=None),
}


def gen_params(combo, shape):
    """(GenParams, batch) of a combination at a shape"""
    s, stages = SHAPES[shape], COMBOS[combo]
    U, F, A, N = s["num_tx"], s["num_subcarriers"], s["num_rx_ant"], s["fft_size"]
    dmrs_symbols = (2, 3, 10, 11) if U > 2 else (2, 11)      # more than 2 ports need the time cover's pairs
    kw = dict(num_tx=U, num_subcarriers=F, num_rx_ant=A, dmrs_symbols=dmrs_symbols, mcs_bits=(2, 4),
              cdm_group=tuple(u % 2 for u in range(U)), mcs_of_user=tuple(-1 if u % 2 == 0 else 1 for u in range(U)),
              num_taps=s["num_taps"], seed=77)
    if "chan" in stages:
        kw.update(user_profiles=[(100e-9 * (1 + u % 3), 100.0 * (1 + u % 4)) for u in range(U)],
                  rx_corr=rx_correlation(A, 0.9))
    if "cfo" in stages:
        kw.update(cfo_hz=[300.0 * (u + 1) for u in range(U)], fft_size=N, h_with_phase=True)
    if "dmrs" in stages:
        kw.update(dmrs=DMRSPorts.default(U))
    for steps in (1, 14):
        if f"cir{steps}" in stages:
            E, L = 5, 3
            rng = np.random.default_rng(steps)
            a = rng.standard_normal((E, A, L, steps)) + 1j * rng.standard_normal((E, A, L, steps))
            kw.update(cir=CIRChannel(CIRDataset(a, np.sort(rng.uniform(0.0, 5e-7, (E, L)), axis=-1)), select="random"))
    if "td" in stages:
        kw.update(td=TimeDomain(fft_size=N, cp=s["cp"], delay=[u % 3 for u in range(U)], pa_ibo_db=6.0,
                                h_with_delay=True))
    if "tc" in stages:
        kw.update(tc=TimeChannelParams(fft_size=N, cp=s["cp"], l_min=-2, l_max=3, timing_advance=1))
    return GenParams(**kw), s["batch"]
