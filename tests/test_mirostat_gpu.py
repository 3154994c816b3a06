"""csrc/kernels/mirostat.hip against the yardsticks of tests/_mirostat_cases.py: survivors by two-sided containment
against fp64, mu after one update within EPS_MU, every element the kernels must not touch bit for bit; on the DFA of
the Llama-3 vocabulary too, and twice in a row for the same bits."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mirostat_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("rows", ["perm", None])
@pytest.mark.parametrize("vocab", [1003, 5003])
def test_ladder_cases(vocab, rows, dt):
    mc.check(mc.ladder_case(vocab, dt, rows), DEV)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("vocab,rows", [(1003, "perm"), (5003, None), (128256, "perm")])
def test_random_rows(vocab, rows, T, dt):
    mc.check(mc.random_case(vocab, dt, T, rows, seed=int(T * 2) + (vocab % 7)), DEV)


def test_nout_not_advanced_moves_no_mu():
    mc.check(mc.ladder_case(1003, "bf16"), DEV, sample=False)
    mc.check(mc.random_case(5003, "f32", 1.0, "perm", seed=3), DEV, sample=False)


def test_the_whole_module_as_on_the_reference_path():
    mc.check_all(DEV, big=False)


def test_same_row_same_bits_on_every_launch():
    c = mc.random_case(128256, "bf16", 1.0, "perm", seed=20)
    a, b = c.run(DEV), c.run(DEV)
    for k in ("buf", "mu", "m", "lnz", "mark", "out"):
        assert mc.tc.same_bits(a[k], b[k]) if a[k].is_floating_point() else torch.equal(a[k], b[k]), k


def test_many_slots_update_grid():
    """200 slots: the update kernel's slots-per-workgroup indexing past one workgroup, and its tail."""
    g = torch.Generator().manual_seed(9)
    nxt, dist = mc.tc.build_dfa(1003, g)
    legal = mc.tc.legal_mask(nxt, dist, mc.ST_GEN, mc.REMAINING)
    x = mc.tc.random_rows(1003, "bf16", g, n=4)
    sl = []
    for i in range(200):
        if i % 9 == 4:
            sl.append(mc.slot("parked"))
        else:
            sl.append(mc.slot(x=x[i % 4], T=(0.5, 1.0, 2.0)[i % 3], on=int(i % 5 != 0), tau=1.0 + i % 4, eta=0.25,
                              mu=mc.midway_mu(x[i % 4], legal, (0.5, 1.0, 2.0)[i % 3], 0.05 + 0.004 * i), nout=i % 3))
    mc.check(mc.Case("200 slots", 1003, "bf16", nxt, dist, sl), DEV)


def test_input_checks_name_a_bad_row_before_the_launch():
    from chronos import ops

    c = mc.ladder_case(1003, "f32")
    c.row[0] = 99
    ops.set_input_checks(True)
    try:
        with pytest.raises(IndexError, match="row"):
            c.run(DEV)
    finally:
        ops.set_input_checks(os.environ.get("CHRONOS_CHECK_INPUTS", "0") not in ("", "0"))
