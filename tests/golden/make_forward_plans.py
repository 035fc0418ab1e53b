"""Record tests/golden/forward_plans.json: the per-kernel launch counts of executed f16 forwards over the table of
tests/test_forward_plan.py, from whichever library ``NRX_LIB_PATH`` names (default: the in-tree build).  Needs an
MI355X; uses only CGNNEngine.update_schedule / fused_config / profile / profile_read, so it runs against a library
from before ``plan_forward`` (build one beside the tree with build.build(lib=..., obj_dir=...) from that commit):

    NRX_LIB_PATH=/path/to/parent/libnrx.so python tests/golden/make_forward_plans.py --commit <parent commit>

``--out FILE`` writes elsewhere.  Random inputs and seeded weights: the schedule depends on shapes only.
"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from neural_rx_amd import _lib                                                       # noqa: E402
from tests.helpers import make_case, run_engine                                      # noqa: E402
from tests.test_forward_plan import (BASELINE, DEFAULT_MASK, GOLDEN, SHAPES, combos, shape_key,   # noqa: E402
                                     spec_of)


def case_of(shape, seed=1):
    topology, ant, users, prbs, batch = shape
    rng = np.random.default_rng(seed)
    return make_case(topology, batch=batch, users=users, prbs=prbs, num_rx_ant=ant, seeded_weights=True,
                     random_inputs=True, seed=seed, mcs_choice=rng.integers(0, spec_of(shape).num_mcs, (batch, users)))


def launch_counts(eng, case, num_it, fused, mask):
    """profiler counts, in the order of _lib.KERNELS, of one forward"""
    case.num_it = num_it
    eng.update_schedule(mask)
    eng.fused_config(enable=fused)
    eng.profile(True)
    run_engine(case, "f16", eng)
    prof = eng.profile_read()
    eng.profile(False)
    eng.check()
    return [prof[k][0] for k in _lib.KERNELS]


def main(argv):
    from neural_rx_amd.receiver import CGNNEngine
    out = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN
    commit = argv[argv.index("--commit") + 1] if "--commit" in argv else "unknown"
    lib = _lib.load()
    data = {"recorded_from": {"commit": commit, "build_id": lib.nrx_build_id().decode(), "cus": 256, "xccs": 8},
            "kernels": _lib.KERNELS, "cases": {}, "baseline": {}}
    for shape in SHAPES + BASELINE:
        case = case_of(shape)
        eng = CGNNEngine(case.spec, case.weights)
        try:
            if shape in SHAPES:
                data["cases"][shape_key(shape)] = [launch_counts(eng, case, *c) for c in combos(shape)]
            if shape in BASELINE:
                data["baseline"][shape_key(shape)] = launch_counts(eng, case, case.spec.num_it, 1, DEFAULT_MASK)
        finally:
            eng.close()
        print(shape_key(shape), flush=True)
    with open(out, "w", encoding="utf-8") as f:
        # one line per forward: its nine counts
        f.write(re.sub(r"\[\s+((?:\d+,\s+)*\d+)\s+\]", lambda m: "[" + re.sub(r"\s+", "", m.group(1)) + "]",
                       json.dumps(data, indent=1, sort_keys=True)))
        f.write("\n")
    print(f"{out}: {len(data['cases'])} + {len(data['baseline'])} shapes from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main(sys.argv[1:])
