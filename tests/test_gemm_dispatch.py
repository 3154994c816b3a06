"""The projection GEMM dispatch (ops.linear / gate_up_silu / gemv_resid / resid_ok / qkv_rope) against the recorded
launch log of tests/golden/gemm_dispatch.json: per (entry point, shape, weights, x, switches) and M, which op is
launched with which mode, config, split-K, operands, optional arguments and eps, what the ``w4_stats`` counters add,
what raised and what was returned (tests/_gemm_dispatch.py).  CPU-only: a recorder stands in for the extension.  The
file is the definition of "routing unchanged": it is regenerated only when a route is changed on purpose."""
import json

import _gemm_dispatch as D


def _runs_full(result, case):
    return [[lo, hi, result["logs"][i]] for lo, hi, i in result["cases"][case]]


def test_dispatch_matches_the_golden_launch_log():
    with open(D.GOLDEN) as fh:
        want = json.load(fh)
    got = D.collect()
    assert list(got["cases"]) == list(want["cases"]), "the grid of cases differs from the golden file's"
    print(f"{len(got['cases'])} cases, {len(got['logs'])} distinct logs")
    for case in want["cases"]:
        g, w = _runs_full(got, case), _runs_full(want, case)
        if g != w:
            first = next((a, b) for a, b in zip(g + [None], w + [None]) if a != b)
            print(f"first differing case: {case}\n  live run:   {json.dumps(first[0])}\n  golden run: {json.dumps(first[1])}")
            print("  live:   " + json.dumps(g) + "\n  golden: " + json.dumps(w))
        assert g == w, f"dispatch differs from the golden launch log in case {case}"
