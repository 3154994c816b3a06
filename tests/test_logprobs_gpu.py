"""The per-token logprob kernels (csrc/kernels/logprobs.hip) at the smallest shapes that can break them: vocabularies
that are no multiple of 8 / of the workgroup, bf16 and fp32 logits with a padded row stride, K in {1, 5, 20}, the five
kinds of slot that must be left alone, tie plateaus across the K-th place, and the commit kernel's write guards.
Cases, expected values and the tolerance are in tests/_logprobs_cases.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _logprobs_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = [c for c in lc.cases() if c[0] < 5000]


@pytest.mark.parametrize("case", lc.cases(), ids=lc.case_id)
def test_token_logprobs(case):
    lc.check_pre(*case, "cuda")


@pytest.mark.parametrize("case", SMALL, ids=lc.case_id)
def test_commit(case):
    lc.check_commit(*case, "cuda")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_commit_full_ring_writes_nothing(dt):
    lc.check_commit_full_ring(1000, dt, 5, "cuda")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_chain_with_sampler(dt):
    lc.check_chain(4104, dt, 5, "cuda")
