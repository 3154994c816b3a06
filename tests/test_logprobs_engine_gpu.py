"""Per-token logprobs through the engine on the GPU (tiny model): the checks of tests/test_logprobs_engine.py on the
HIP kernels (eager, with the sampler recorder), and a graph-captured run that must equal the eager run bit for bit."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _logprobs_engine as le  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_plain_run(monkeypatch):
    eng, reqs = le.check_run(DEV, monkeypatch, le.plain_subs())
    assert reqs[2].logprobs == 5 and all(len(top) <= 5 for _, top in reqs[2].out_logprobs)


def test_more_requests_than_slots_compaction(monkeypatch):
    le.check_run(DEV, monkeypatch, le.compaction_subs(), expect_stat="compactions")


def test_lazy_kv_preemption(monkeypatch):
    subs = le.preemption_subs()
    nb = le.preemption_blocks(DEV, subs)
    eng, reqs = le.check_run(DEV, monkeypatch, subs, expect_stat="preemptions", kv_alloc="lazy", kv_blocks=nb,
                             kv_watermark=0.0, kv_lookahead=16, mixed_batching=False)
    assert any(r.preemptions for r in reqs)


def test_mixed_batching_some_want_logprobs(monkeypatch):
    le.check_mixed(DEV, monkeypatch)


def test_jump_forward_is_suppressed():
    le.check_jump_suppressed(DEV)


def test_engine_never_asked_allocates_and_launches_nothing():
    le.check_never_asked(DEV)


def test_graph_run_equals_eager_run_bit_for_bit():
    subs = le.plain_subs() + le.compaction_subs()
    eager_eng = le.engine(DEV, use_graphs=False)
    eager = le.run(eager_eng, subs)
    graph_eng = le.engine(DEV, use_graphs=True)
    graph = le.run(graph_eng, subs)
    assert any(len(k) == 4 for k in graph_eng._graphs), "the logprob variant of a decode graph was captured"
    assert graph_eng.stats["logprob_launches"] == eager_eng.stats["logprob_launches"] > 0
    for a, b in zip(eager, graph):
        assert a.out_ids == b.out_ids
        assert len(b.out_logprobs) == len(b.out_ids) > 0
        assert a.out_logprobs == b.out_logprobs  # floats compared exactly
