"""Mirostat 2.0 through the engine on the GPU (tiny model, HIP kernels): the trajectory, jump-forward, preemption and
slot-reuse checks of tests/test_mirostat.py run eagerly on the device, and a graph-captured run — the mirostat variant
of the decode graph captured and replayed in k-step bursts — must equal the eager run token for token and in its final
mu bit for bit."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mirostat_engine as me  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_trajectory_replayed_from_logprobs():
    me.check_trajectory(DEV)


def test_jump_forward_leaves_mu_alone(monkeypatch):
    me.check_jump_forward(DEV, monkeypatch)


def test_preemption_resumes_from_the_saved_mu(monkeypatch):
    me.check_preemption(DEV, monkeypatch)


def test_slot_reuse_resets_flag_and_mu(monkeypatch):
    me.check_slot_reuse(DEV, monkeypatch)


def test_graph_bursts_equal_the_eager_run_tokens_and_mu_bit_for_bit():
    me.check_graph_equals_eager(DEV)


def test_mixed_batch_under_graphs_leaves_the_other_requests_token_identical():
    eng, _ = me.check_mixed(DEV, use_graphs=True)
    assert any(k[-1] == "mi" for k in eng._graphs), "a mirostat variant of a decode graph"


def test_engine_never_asked_allocates_nothing_and_keeps_its_graph_keys():
    eng, _ = me.check_never_asked(DEV, use_graphs=True)
    assert eng._graphs, "decode graphs were captured"
