"""Static instruction-class counts of kernels in a gfx950 assembly listing, per barrier-delimited phase.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S neural_rx_amd/csrc/nrx_k_col.hip -o col.s
    python tools/insn_classes.py col.s k_update_col [--json]

Every kernel whose (mangled) name contains the given substring gets one row per phase (the code between two
workgroup barriers) and a total.  The classes go by mnemonic prefix only:

    mfma    v_mfma*                                    matrix pipe
    dw      v_pk_mul_f16 / v_pk_fma_f16 and every DPP form: the depthwise 3x3
    arith   conversions, packs, permlane swaps, max, float / double add, mul, fma: arithmetic of the result
    valu    every other v_*: moves, selects, compares, integer and address arithmetic, bit operations
    salu    every s_* (branches and waits included)
    lds     ds_*
    vmem    global_* / buffer_* / flat_* / scratch_*

The kernels are nearly straight-line, so a static count is close to what a wave executes; code behind a branch that a
shape never takes (a fallback store path) still counts.  It is a comparison tool: the same listing before and after a
change, never an absolute.
"""
import json
import re
import sys

CLASSES = ["mfma", "dw", "arith", "valu", "salu", "lds", "vmem"]
ARITH = ("v_cvt", "v_pack", "v_perm", "v_pk_max", "v_max", "v_min", "v_pk_add_f", "v_pk_mul_f32", "v_pk_fma_f32",
         "v_add_f", "v_sub_f", "v_mul_f", "v_fma", "v_mac_f", "v_fmac_f", "v_mad_f", "v_rcp", "v_rsq", "v_sqrt",
         "v_div", "v_ldexp", "v_frexp", "v_trunc", "v_rndne", "v_fract", "v_floor", "v_ceil")


def classify(mn, line):
    if mn.startswith("v_mfma") or mn.startswith("v_smfma"):
        return "mfma"
    if mn.startswith(("ds_",)):
        return "lds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("v_"):
        if "dpp" in mn or "row_shr" in line or "row_shl" in line or "quad_perm" in line or "row_bcast" in line:
            return "dw"
        if mn.startswith(("v_pk_mul_f16", "v_pk_fma_f16")):
            return "dw"
        if mn.startswith(ARITH):
            return "arith"
        return "valu"
    return None


def kernels(path):
    """{name: [instruction lines]} of the functions of an assembly listing"""
    out, cur = {}, None
    with open(path, encoding="utf-8", errors="replace") as f:
        for line in f:
            m = re.match(r"^([A-Za-z_][\w$.]*):", line)
            if m and not m.group(1).startswith(".L"):
                cur = m.group(1)
                out[cur] = []
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
            if cur and line.startswith("\t"):
                t = line.strip()
                if t and not t.startswith((".", ";")):
                    out[cur].append(t)
    return {k: v for k, v in out.items() if v}


def count(lines):
    """[per-phase {class: n}] + the total as the last entry"""
    phases = [dict.fromkeys(CLASSES, 0)]
    for t in lines:
        mn = t.split()[0]
        c = classify(mn, t)
        if c is None:
            continue
        phases[-1][c] += 1
        if c == "salu" and mn.endswith("barrier"):
            phases.append(dict.fromkeys(CLASSES, 0))
    total = {c: sum(p[c] for p in phases) for c in CLASSES}
    return phases, total


def main(argv):
    path, pat = argv[1], argv[2]
    res = {}
    for name, lines in kernels(path).items():
        if pat in name:
            phases, total = count(lines)
            res[name] = {"phases": phases, "total": total}
    if "--json" in argv:
        print(json.dumps(res, indent=1))
        return
    for name, r in res.items():
        print(name)
        print("  %-8s" % "phase" + "".join("%8s" % c for c in CLASSES))
        for i, p in enumerate(r["phases"]):
            print("  %-8d" % i + "".join("%8d" % p[c] for c in CLASSES))
        print("  %-8s" % "total" + "".join("%8d" % r["total"][c] for c in CLASSES))


if __name__ == "__main__":
    main(sys.argv)
