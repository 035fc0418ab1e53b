"""Executed = planned: the per-kernel profile of one executed f16 forward equals the plan ``nrx_debug_forward_plan``
returns for the current device (cus = 0), over threshold cases of tests/test_forward_plan.py (at most 130 slots of 4 or
5 PRB: every forward stays under a millisecond)."""
import pytest

from neural_rx_amd import _lib
from tests.golden.make_forward_plans import case_of, launch_counts
from tests.test_forward_plan import check_records, counts, plan, shape_key

pytestmark = pytest.mark.gpu

# (shape, num_it, fused, mask)
CASES = [
    (("nrx_rt", 4, 1, 4, 42), 2, 1, 29),              # P16S
    (("nrx_rt", 4, 1, 4, 85), 2, 1, 29),              # P16M
    (("nrx_rt", 4, 1, 4, 86), 2, 1, 29),              # neither small tier: one-item column launches
    (("nrx_rt", 4, 2, 4, 128), 2, 1, 0),              # strip kernels, paired aggregation and readout
    (("nrx_rt", 4, 2, 4, 130), 2, 1, 0),              # ... unpaired (items % 16)
    (("nrx_rt", 4, 2, 4, 129), 2, 1, 29),             # looping column kernels
    (("nrx_rt", 4, 2, 4, 128), 2, 1, 29 | 32),        # k_fwd_col
    (("nrx_rt", 4, 2, 4, 129), 2, 1, 29 | 32),        # ... out: more items than CUs
    (("nrx_large", 4, 2, 4, 128), 3, 1, 0),           # k_forward by default (four stages, no column launches)
    (("nrx_rt", 4, 2, 5, 128), 2, 1, 29),             # two column strips: RR aggregation, strip readout
    (("nrx_rt", 4, 2, 5, 128), 2, 1, 29 | 64),        # ... column updates on the wide grid
    (("nrx_rt", 4, 3, 4, 128), 2, 2, 29),             # k_forward with combine stages
    (("nrx_rt", 4, 3, 4, 128), 2, 0, 3),              # RR updates and combine launches
    (("nrx_rt", 16, 2, 4, 128), 2, 1, 29),            # 2A = 32: strip StateInit, ch32 column updates
    (("nrx_rt_var_mcs", 4, 2, 4, 128), 2, 1, 29),     # two StateInit launches, two LLR heads: strip readout
]


@pytest.mark.parametrize("shape,num_it,fused,mask", CASES,
                         ids=["%s it%d f%d m%d" % (shape_key(c[0]), c[1], c[2], c[3]) for c in CASES])
def test_profile_of_a_forward_equals_its_plan(shape, num_it, fused, mask):
    import torch
    from neural_rx_amd.receiver import CGNNEngine
    case = case_of(shape)
    eng = CGNNEngine(case.spec, case.weights)
    try:
        got = launch_counts(eng, case, num_it, fused, mask)
    finally:
        eng.close()
    chunks = plan(_lib.load(), shape, num_it, mask, fused, cus=0, xccs=0)
    assert got == counts(chunks), chunks
    check_records(chunks, shape[4], shape[2], torch.cuda.get_device_properties(0).multi_processor_count)
