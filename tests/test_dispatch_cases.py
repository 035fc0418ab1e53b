"""tests/dispatch_cases.py against the launchers it describes; no GPU.

Two checks.  (1) The labels of every listed host dispatcher -- ``case N:`` / ``default:`` of each ``switch``, doubled
where the label's statement passes ``vec`` on, or the instantiations an if-chain returns -- are read from the
source text, and every one has an entry in the table (and the table names no label the source does not have).
(2) Every entry names a test function that exists, and its parameter values are a row of that function's
``parametrize`` lists.  So a new instantiation cannot land without a value test naming it, and a case cannot leave
a case table while the table still points at it.  The source is read for labels only.
"""
import importlib
import os
import re

import pytest

from tests import dispatch_cases as DC

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "neural_rx_amd", "csrc")


def _block(text, start):
    """text[start] is '{': the index one past its matching '}'"""
    depth = 0
    for i in range(start, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return i + 1
    raise AssertionError("unbalanced braces")


def function_body(text, name):
    """the body of the one definition of ``name`` (a line at column 0 that ends in '{')"""
    found = [m for m in re.finditer(r"^[A-Za-z_][^\n;]*\b%s\([^;{]*\)\s*\{" % re.escape(name), text, re.M)]
    assert len(found) == 1, (name, len(found))
    return text[found[0].end() - 1:_block(text, found[0].end() - 1)]


def labels_of(body):
    """[set of labels] per dispatch site of a launcher's body: one set per ``switch``; without a switch, the
    instantiations its ``return`` statements launch"""
    out = []
    for m in re.finditer(r"\bswitch\s*\([^)]*\)\s*\{", body):
        sw = body[m.end() - 1:_block(body, m.end() - 1)]
        marks = list(re.finditer(r"\b(case\s+\w+|default)\s*:", sw))
        labels = set()
        for k, mk in enumerate(marks):
            stmt = sw[mk.end():marks[k + 1].start() if k + 1 < len(marks) else len(sw)]
            label = " ".join(mk.group(1).split())
            if re.search(r"\bvec\b", stmt):
                labels |= {(label, "vec"), (label, "scalar")}
            else:
                labels.add(label)
        out.append(labels)
    if not out:
        out.append(set(re.findall(r"\breturn\s+(\w+<[^;()]*>)\(", body)))
    return out


def _source(fname):
    with open(os.path.join(CSRC, fname), encoding="utf-8") as f:
        return f.read()


def test_the_parser_on_a_known_launcher():
    body = function_body(_source("nrx_lmmse.hip"), "launch_lmmse")
    (labels,) = labels_of(body)
    assert ("case 1", "vec") in labels and ("case 8", "scalar") in labels and "default" in labels
    assert len(labels) == 17
    (chain,) = labels_of(function_body(_source("nrx_timechan.hip"), "launch_tc_args"))
    assert chain == {"launch_tc_k<4, 4>", "launch_tc_k<8, 2>", "launch_tc_k<16, 1>"}
    assert [len(s) for s in labels_of(function_body(_source("nrx_softmetrics.hip"), "launch_llr_stats"))] == [5, 5]


@pytest.mark.parametrize("launcher", sorted(DC.DISPATCH))
def test_every_label_has_an_entry(launcher):
    fname, _, tables = DC.DISPATCH[launcher]
    sites = labels_of(function_body(_source(fname), launcher))
    assert len(sites) == len(tables), (launcher, len(sites), len(tables))
    for labels, table in zip(sites, tables):
        assert labels, launcher
        missing, stale = labels - set(table), set(table) - labels
        assert not missing, f"{launcher}: no value test named for {sorted(map(str, missing))}"
        assert not stale, f"{launcher}: the table names labels the source does not have: {sorted(map(str, stale))}"


def _entries():
    for launcher, (_, _, tables) in DC.DISPATCH.items():
        for table in tables:
            for label, t in table.items():
                yield f"{launcher} {label}", t
    for (launcher, branch), t in DC.BRANCHES.items():
        yield f"{launcher} {branch}", t


def _rows(fn):
    """per parametrize mark of a test function: (argument names, list of value tuples)"""
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = mark.args[0]
        names = [n.strip() for n in names.split(",")] if isinstance(names, str) else list(names)
        rows = []
        for v in mark.args[1]:
            if hasattr(v, "marks"):                              # a pytest.param(...)
                v = v.values if len(names) > 1 else v.values[0]
            rows.append(tuple(v) if len(names) > 1 else (v,))
        yield names, rows


def test_every_entry_names_a_case_that_exists():
    n = 0
    for what, t in _entries():
        mod = importlib.import_module(t.module)
        fn = getattr(mod, t.function, None)
        assert callable(fn), f"{what}: {t.module} has no {t.function}"
        left = dict(t.params)
        for names, rows in _rows(fn):
            mine = [k for k in names if k in left]
            if not mine:
                continue
            idx = [names.index(k) for k in mine]
            assert any(all(r[i] == left[k] for i, k in zip(idx, mine)) for r in rows), \
                f"{what}: {t.function} has no case with " + ", ".join(f"{k} = {left[k]!r}" for k in mine)
            for k in mine:
                del left[k]
        assert not left, f"{what}: {t.function} is not parametrised over {sorted(left)}"
        n += 1
    assert n >= 80


def test_the_listed_dispatchers():
    assert set(DC.DISPATCH) == {"launch_lmmse", "launch_kbest", "launch_chest_lmmse", "launch_chest_lmmse3",
                                "launch_ls_estimate", "launch_llr_stats", "launch_count_errors", "launch_tc_args",
                                "launch_n"}
