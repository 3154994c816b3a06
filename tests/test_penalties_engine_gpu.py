"""Penalties through the engine on the GPU (tiny model, HIP kernels): the checks of tests/test_penalties_engine.py,
and a graph-captured run that must equal the eager run token for token."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _penalty_engine as pe  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_plain_run_mixed_penalised_and_unpenalised():
    pe.check_run(DEV, pe.plain_subs())


def test_more_requests_than_slots_compaction():
    pe.check_run(DEV, pe.compaction_subs(), expect_stat="compactions")


def test_lazy_kv_preemption_keeps_the_history():
    subs = pe.preemption_subs()
    nb = pe.preemption_blocks(DEV, subs)
    eng, reqs = pe.check_run(DEV, subs, expect_stat="preemptions", kv_alloc="lazy", kv_blocks=nb, kv_watermark=0.0,
                             kv_lookahead=16, mixed_batching=False)
    assert any(r.preemptions for r in reqs)


def test_mixed_batching():
    pe.check_mixed(DEV)


def test_jump_forward_runs_enter_the_history():
    pe.check_jump_forward(DEV)


def test_presence_penalty_property():
    pe.check_presence_property(DEV)


def test_neutral_requests_untouched_and_never_asked():
    pe.check_neutral_untouched(DEV)


def test_slot_reuse_resets_the_state():
    pe.check_slot_reuse(DEV)


def test_graph_run_equals_eager_run():
    subs = pe.plain_subs() + pe.compaction_subs()
    eager_eng = pe.engine(DEV, use_graphs=False)
    eager = pe.run(eager_eng, subs)
    graph_eng = pe.engine(DEV, use_graphs=True)
    graph = pe.run(graph_eng, subs)
    assert any(len(k) == 5 and k[-1] == "pen" for k in graph_eng._graphs), "a penalty variant of a decode graph"
    assert graph_eng.stats["penalty_launches"] == eager_eng.stats["penalty_launches"] > 0
    for a, b in zip(eager, graph):
        assert a.out_ids == b.out_ids and a.text == b.text
