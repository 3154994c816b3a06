"""min_p / typical_p through the engine on the GPU (tiny model, HIP kernels, decode_burst 4): the recorder checks of
tests/test_truncate.py run eagerly, and a graph-captured run — the truncation variant of the decode graph captured
and replayed — must equal the eager run token for token."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _truncate_engine as te  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_minp_one_picks_a_maximal_legal_logit_at_every_step(monkeypatch):
    te.check_minp1(DEV, monkeypatch)


def test_mixed_batch_typical_p_in_the_widened_set_and_neighbours_token_identical(monkeypatch):
    te.check_mixed(DEV, monkeypatch)


def combined_subs():
    p = te.prompts(3, seed=12)
    return [(p[0], te.sampled(fmt=te.VERDICT_SCHEMA, num_predict=30, min_p=0.2, logprobs=2)),
            (p[1], te.sampled(fmt=None, num_predict=16, min_p=0.2, repeat_penalty=1.3, presence_penalty=0.5, seed=4)),
            (p[2], dict(fmt=te.VERDICT_SCHEMA, num_predict=30))]


def test_logprobs_and_penalties_combine_with_minp(monkeypatch):
    eng = te.engine(DEV)
    rec = te.Recorder(eng, monkeypatch)
    lp, pen, greedy = te.run(eng, combined_subs())
    # logprobs are taken before truncation: one entry per token, and the chosen token's logprob is finite
    assert len(lp.out_logprobs) == len(lp.out_ids) > 0
    assert all(v > float("-inf") for v, _ in lp.out_logprobs)
    te.check_minp_request(rec, lp, 0.2)
    # the recorded rows of the penalised request are the penalised ones: min_p keys off them
    assert pen.penalty and te.check_minp_request(rec, pen, 0.2) > 0
    assert eng.stats["penalty_launches"] > 0 and eng.stats["logprob_launches"] > 0
    assert eng.stats["truncate_launches"] > 0 and not rec.steps(greedy)


def test_graph_run_equals_eager_run_token_for_token():
    subs = te.minp1_subs() + te.mixed_subs() + combined_subs()
    eager_eng = te.engine(DEV, use_graphs=False, max_slots=16)
    eager = te.run(eager_eng, subs)
    graph_eng = te.engine(DEV, use_graphs=True, max_slots=16)
    graph = te.run(graph_eng, subs)
    assert any(k[-1] == "tr" and len(k) == 6 for k in graph_eng._graphs), "a truncation variant of a decode graph"
    assert graph_eng.stats["truncate_launches"] == eager_eng.stats["truncate_launches"] > 0
    for a, b in zip(eager, graph):
        assert a.out_ids == b.out_ids and a.text == b.text
        assert a.out_logprobs == b.out_logprobs


def test_engine_never_asked_launches_nothing_and_keeps_its_graph_keys():
    eng = te.check_never_asked(DEV, use_graphs=True)
    assert eng._graphs, "decode graphs were captured"


def test_slot_reuse_resets_the_parameters():
    te.check_slot_reuse(DEV)
