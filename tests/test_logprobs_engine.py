"""Per-token logprobs through the engine on the CPU path (tiny model, eager): every reported entry against the test's
own formula on the recorded sampler inputs, tokens unchanged by asking, through compaction, preemption and mixed
steps.  Helpers: tests/_logprobs_engine.py; the same checks run on the GPU in tests/test_logprobs_engine_gpu.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _logprobs_engine as le  # noqa: E402

DEV = "cpu"


def test_plain_run(monkeypatch):
    eng, reqs = le.check_run(DEV, monkeypatch, le.plain_subs())
    assert reqs[2].logprobs == 5 and all(len(top) <= 5 for _, top in reqs[2].out_logprobs)
    assert all(top == [] for _, top in reqs[1].out_logprobs)


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
