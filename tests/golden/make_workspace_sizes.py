"""Record tests/golden/workspace_sizes.json: what every ``*_workspace_size`` entry point answers over the table of
tests/test_workspace_sizes.py, from whichever library ``NRX_LIB_PATH`` names (default: the in-tree build).

    python tests/golden/make_workspace_sizes.py          the entry points that need no handle ("cpu")
    python tests/golden/make_workspace_sizes.py --gpu    the handle-bound ones ("gpu"; needs an MI355X)

Each run replaces its own section and keeps the other.  ``--out FILE`` writes elsewhere.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from neural_rx_amd import _lib                                   # noqa: E402
from tests.test_workspace_sizes import GOLDEN, sizes_cpu, sizes_gpu   # noqa: E402


def main(argv):
    out = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN
    data = {"cpu": {}, "gpu": {}}
    for path in (GOLDEN, out):
        if os.path.exists(path):
            with open(path, encoding="utf-8") as f:
                data.update(json.load(f))
    lib = _lib.load()
    section = "gpu" if "--gpu" in argv else "cpu"
    data[section] = (sizes_gpu if section == "gpu" else sizes_cpu)(lib)
    with open(out, "w", encoding="utf-8") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(data[section])} {section} sizes from {_lib.LIB_PATH} ({lib.nrx_build_id().decode()})")


if __name__ == "__main__":
    main(sys.argv[1:])
