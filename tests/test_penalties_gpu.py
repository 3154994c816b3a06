"""The penalty kernel (csrc/kernels/penalties.hip) at the smallest shapes that can break it: logits widths that are and
are not a multiple of 8, one 2-row case at the Llama-3 width, 1 to 9 slots, bf16 and fp32 rows with a padded stride,
windows of 1, 64 and the 1024 cap, histories that straddle the prompt tail and the output ring, and the slots that
must be left alone.  Cases, oracle and tolerance are in tests/_penalty_cases.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _penalty_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", pc.cases(), ids=pc.case_id)
def test_apply_penalties_kernel(case):
    pc.check(case, "cuda")
