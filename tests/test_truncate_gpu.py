"""csrc/kernels/truncate.hip against the yardsticks of tests/_truncate_cases.py: min_p bit for bit against the
reference, typical_p exactly on constructed rows and by two-sided containment on random ones, and the sampler on
truncated rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _truncate_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def bank():
    from chronos.brain.constrain import GrammarBank
    from chronos.brain.tokenizer import load_tokenizer
    from chronos.sensor.prompt import VERDICT_SCHEMA

    tok = load_tokenizer(None)
    b = GrammarBank(tok.token_bytes_list(), tok.stop_ids, 128256, 512, "cpu")
    free, verdict = b.get(None).start, b.get(VERDICT_SCHEMA).start
    return b.next[:b.used].clone(), b.dist[:b.used].clone(), free, verdict


@pytest.mark.parametrize("n", [1, 3, 64])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("vocab", [1003, 128256])
def test_minp_row_equals_the_reference_bit_for_bit(vocab, dt, n):
    tc.check_minp(n, vocab, dt, DEV)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("vocab", [1003, 128256])
def test_minp_without_row_of_slot(vocab, dt):
    tc.check_minp(3, vocab, dt, DEV, rows=None, seed=1)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("grammar", ["free", "verdict"])
def test_minp_on_the_grammar_bank(bank, grammar, dt):
    nxt, dist, free, verdict = bank
    start = free if grammar == "free" else verdict
    assert int(tc.legal_mask(nxt, dist, start, 60).sum()) > 1
    tc.check_minp(3, 128256, dt, DEV, nxt=nxt, dist=dist, live_state=start, seed=2, remaining=60)


@pytest.mark.parametrize("with_minp", [False, True])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("vocab", [1003, 128256])
def test_typical_p_on_constructed_rows_is_exact(vocab, dt, with_minp):
    tc.check_typical_ladder(vocab, dt, DEV, with_minp)


@pytest.mark.parametrize("tp", [0.2, 0.5, 0.9])
@pytest.mark.parametrize("dt,seed", [("bf16", 1), ("f32", 2)])
def test_typical_p_on_random_rows_is_contained(dt, seed, tp):
    tc.check_typical_random(dt, DEV, tp, seed)


def test_typical_p_is_reproducible():
    """Mass is accumulated in integers: two launches on the same rows write the same bits."""
    g = torch.Generator().manual_seed(5)
    nxt, dist = tc.build_dfa(128256, g)
    c = tc.Slots(3, 128256, "bf16", DEV, nxt, dist, tc.ST_GEN, list(tc.random_rows(128256, "bf16", g)), minp=(0.01,),
                 typ=(0.6,))
    assert tc.same_bits(c.run(), c.run())


def test_sampler_after_truncation_draws_a_survivor():
    tc.check_sampler_after(DEV)
