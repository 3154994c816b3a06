"""The repeat / frequency / presence penalty op on the CPU reference (chronos.ops.reference.apply_penalties) against
the plain Python loop of tests/_penalty_cases.py: cases, oracle and tolerance are there."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _penalty_cases as pc  # noqa: E402

CASES = pc.cases()


@pytest.mark.parametrize("case", CASES, ids=pc.case_id)
def test_apply_penalties_reference(case):
    pc.check(case, "cpu")


def test_cases_penalise_something():
    """The cases are not vacuous: the dead / neutral ones aside, each has penalised logits, and the set covers both
    dtypes, strided views, row permutations and the window cap."""
    assert {c["dt"] for c in CASES} == {"bf16", "f32"}
    assert any(c["full"] is not c["logits"] for c in CASES) and any(c["row_of_slot"] is not None for c in CASES)
    assert any(c["pen_tail"].shape[1] == pc.CAP for c in CASES)
    for c in CASES:
        n = sum(len(set(t for t in pc.history(c, s) if 0 <= t < c["width"]))
                for s in range(c["state"].numel()) if pc.live(c, s)[0])
        assert (n > 0) == (c["name"] != "no_history"), pc.case_id(c)
