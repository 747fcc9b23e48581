"""The four k-column solves (solve_multi, solve_multi_pc, solve_shifted, solve_minres) against a recording of what they returned
BEFORE their verification norms (k_column_norms, csrc/cgx_multi.hip), result fillers and argument checks were folded into one:
tests/golden/column_results_parent.json, written by tools/record_column_results.py on the MI355X at the commit in front of that
change.  The code under test is so never compared with itself.

Equality bit for bit, no tolerance: X as a digest of its bytes and every field of every result except the wall and event times.
These solves add in fixed orders and use no floating-point atomics, so nothing less is the right bar.  The cases and
why these sizes: the tool's docstring.  The solves run once (record()), the tests share what they returned.
"""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_column_results as rc  # noqa: E402

SOLVES = ("multi", "multi_pc", "shifted", "minres")
CASES = ["n%d/%s" % (n, c) for n in rc.SIZES for c in (
    "multi/nrhs1", "multi/nrhs3", "multi/nrhs16", "multi_pc/jacobi/nrhs3", "multi_pc/pivchol/nrhs3",
    "shifted/dense/1", "shifted/dense/3", "shifted/dense/16", "shifted/csr/3",
    "minres/dense/3", "minres/dense/16", "minres/csr/3", "minres/dense/max_iter0_b0", "minres/dense/max_iter0")]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "column_results_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def now(gpu_pkg):
    return rc.record(gpu_pkg)


def test_the_recording_and_the_run_hold_exactly_the_listed_cases(golden, now):
    assert sorted(golden) == sorted(CASES)
    assert sorted(now) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_same_bits_as_the_recording(golden, now, case):
    assert case in golden, "the fixture lacks %s: record it again at the recording's commit" % case
    want, got = golden[case], now[case]
    assert len(got["results"]) == len(want["results"])
    for j, (w, g) in enumerate(zip(want["results"], got["results"])):
        assert g == w, "%s column %d: %r" % (case, j, {k: (w.get(k), g.get(k)) for k in set(w) | set(g) if w.get(k) != g.get(k)})
    assert got["x_sha256"] == want["x_sha256"], case


def test_the_recording_has_both_ends_of_a_solve(golden):
    """What the cases are chosen for: converged and exhausted columns in every solve, and the max_iter = 0 pair of MINRES."""
    for solve in SOLVES:
        conv = {r["converged"] for c in CASES if "/%s/" % solve in c for r in golden[c]["results"]}
        assert conv == {0, 1}, solve
    for n in rc.SIZES:
        assert [r["converged"] for r in golden["n%d/minres/dense/max_iter0_b0" % n]["results"]] == [1, 1, 1]
        assert [r["converged"] for r in golden["n%d/minres/dense/max_iter0" % n]["results"]] == [0, 0, 0]
        assert all(r["iterations"] == 0 for r in golden["n%d/minres/dense/max_iter0" % n]["results"])
