"""Per-token logprob ops on the CPU path (ops.token_logprobs / ops.token_logprobs_commit -> the fp32 torch reference),
against the expected values of tests/_logprobs_cases.py (its own few lines of torch).  The same cases run on the HIP
kernels in tests/test_logprobs_gpu.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _logprobs_cases as lc  # noqa: E402

SMALL = [c for c in lc.cases() if c[0] < 5000]


@pytest.mark.parametrize("case", lc.cases(), ids=lc.case_id)
def test_token_logprobs(case):
    lc.check_pre(*case, "cpu")


@pytest.mark.parametrize("case", SMALL, ids=lc.case_id)
def test_commit(case):
    lc.check_commit(*case, "cpu")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_commit_full_ring_writes_nothing(dt):
    lc.check_commit_full_ring(1000, dt, 5, "cpu")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_chain_with_sampler(dt):
    lc.check_chain(4104, dt, 5, "cpu")
