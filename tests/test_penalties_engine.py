"""Repeat / frequency / presence penalties through the engine on the CPU (tiny model, reference ops): the
teacher-forced check through a plain run, compaction, preemption, mixed batching and jump-forward; the presence
property; untouched neutral requests.  Helpers and the reasoning behind the skip threshold: tests/_penalty_engine.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _penalty_engine as pe  # noqa: E402

DEV = "cpu"


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


def test_penalty_window_range():
    pe.check_rejects_bad_window(DEV)
