"""The slot generator's memory contract over every stage combination (needs an MI355X).

The generator workspace is several blocks behind one another -- the generator's own, the block of the one
sample-domain stage, the pilot table, the replayed channel (gen_layout, nrx_synth.hip) -- and the size a caller
is told (``nrx_gen_workspace_size_tc``) has to be what the kernels of all of them address.  For each combination
of tests/gen_stages.py at its tiny shape (B 3, U 2, F 24, A 2, 2 taps, FFT 64), with the true channel, the
Aerial outputs and the stage's own output (x' of a td, the received samples of a tc):

  * one call in an oversized zero-filled workspace;
  * one call per fill of tests/memguard.py (0x00, 0xFF = NaN in every float type, 0x7B = large and finite) in the
    body of a guarded buffer of exactly ``workspace_bytes(batch)`` bytes, every output prefilled with 0xFF.

Every ``SlotBatch`` tensor must have the bits of the first call -- a stage that read a workspace byte it had not
written, or wrote one past its block into the next, would not -- and both guard bands must be intact.
"""
import numpy as np
import pytest

from tests.gen_stages import COMBOS, gen_params
from tests.memguard import FILLS, Guarded, same_bits

pytestmark = pytest.mark.gpu

NO, OFFSET = 0.05, 5


def _host(sb):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in vars(sb).items() if v is not None}


@pytest.mark.parametrize("combo", list(COMBOS))
def test_generator_stays_inside_its_workspace(combo):
    import torch
    from neural_rx_amd.generator import SlotGenerator
    p, B = gen_params(combo, "tiny")
    gen = SlotGenerator(p, want_h=True, aerial=True, want_x=True, want_r=True)
    nbytes = gen.workspace_bytes(B)
    assert nbytes > 0
    out = gen(B, NO, slot_offset=OFFSET, workspace=torch.zeros(4 * nbytes + (1 << 20), dtype=torch.uint8, device="cuda"))
    want = _host(out)
    expected = {"y", "h_hat", "active", "mcs_mask", "mcs", "bits", "h", "y_real", "y_imag", "h_ls_real", "h_ls_imag"}
    own = {"cfo": "cfo_eps", "dmrs": "pilots", "td": "x_td", "tc": "r_tc"}
    assert set(want) == expected | {own[s] for s in COMBOS[combo] if s in own}
    for k, v in want.items():
        assert np.isfinite(v).all(), (combo, k)
    for fill in FILLS:
        tag = f"generator {combo} fill {fill:#04x}"
        for v in vars(out).values():
            if v is not None:
                (torch.view_as_real(v) if v.is_complex() else v).view(torch.uint8).fill_(0xFF)
        ws = Guarded(nbytes, fill)
        got = _host(gen(B, NO, slot_offset=OFFSET, out=out, workspace=ws.body))
        ws.check(f"{tag}: workspace of {nbytes} bytes")
        for k in want:
            assert same_bits(got[k], want[k]), (tag, k, "differs from the call in the zero-filled workspace")
