"""Every ctypes ``Structure`` of ``_lib`` against ``include/nrx.h`` as the host C compiler lays it out:
one generated program prints ``sizeof`` of every struct and ``offsetof`` of every field.  No GPU and no
library needed."""
import ctypes
import os
import re
import subprocess

import pytest

from neural_rx_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def structures():
    return {n: c for n, c in vars(_lib).items()
            if n.startswith("nrx_") and isinstance(c, type) and issubclass(c, ctypes.Structure)}


def header_structs():
    """the struct typedefs with a body (the opaque handles have none)"""
    txt = open(os.path.join(INCLUDE, "nrx.h")).read()
    return set(re.findall(r"^typedef\s+struct\s+(nrx_[a-z_0-9]+)\s*\{", txt, re.M))


def test_every_header_struct_has_a_structure():
    assert set(structures()) == header_structs()


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{(struct, field or "size"): bytes} as the C compiler sees the header"""
    lines = []
    for n, cls in sorted(structures().items()):
        lines.append(f'  printf("{n} size %zu\\n", sizeof({n}));')
        lines += [f'  printf("{n} {f} %zu\\n", offsetof({n}, {f}));' for f, *_ in cls._fields_]
    d = tmp_path_factory.mktemp("abi_layout")
    src, exe = d / "layout.c", d / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nrx.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\n  return 0;\n}\n")
    subprocess.run([os.environ.get("CC", "cc"), "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {tuple(l.split()[:2]): int(l.split()[2]) for l in out.splitlines() if l}


def test_sizes_and_offsets_match_the_header(c_layout):
    want = {}
    for n, cls in structures().items():
        want[(n, "size")] = ctypes.sizeof(cls)
        for f, *_ in cls._fields_:
            want[(n, f)] = getattr(cls, f).offset
    assert len(structures()) >= 25 and len(want) >= 334
    bad = {k: (c_layout.get(k), v) for k, v in want.items() if c_layout.get(k) != v}
    assert not bad, bad
    assert set(c_layout) == set(want)
