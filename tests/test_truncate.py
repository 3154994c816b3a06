"""min_p / typical_p on the CPU: the reference semantics of ops.truncate_logits on hand-made rows, the shared cases of
tests/_truncate_cases.py on the reference path, the API options (400s, ``ignored_options``), and the engine on the
tiny model with the recorder of tests/_truncate_engine.py."""
import json
import math
import os
import sys

import pytest
import requests
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _truncate_cases as tc  # noqa: E402
import _truncate_engine as te  # noqa: E402

from chronos import ops  # noqa: E402
from chronos.brain.api.protocol import BadRequest, GenerateParams, penalties_ignored  # noqa: E402

NEG = float("-inf")
DONE = 0


def _dfa(legal_ids, vocab):
    """One live state (1) in which exactly ``legal_ids`` are legal."""
    nxt = torch.full((2, vocab), -1, dtype=torch.int16)
    nxt[1, legal_ids] = 1
    return nxt, torch.tensor([0, 1], dtype=torch.int16)


def _apply(rows, legal_ids, minp, typ, state=None, row_of_slot=None, temp=None):
    x = torch.tensor(rows, dtype=torch.float32)
    n, vocab = x.shape
    nxt, dist = _dfa(legal_ids, vocab)
    before = x.clone()
    ops.truncate_logits(x, None if row_of_slot is None else torch.tensor(row_of_slot, dtype=torch.int32), nxt, dist,
                        DONE, torch.tensor(state or [1] * n, dtype=torch.int32), torch.full((n,), 9, dtype=torch.int32),
                        torch.tensor(temp or [1.0] * n), torch.tensor([math.log(p) if p > 0 else NEG for p in minp]),
                        torch.tensor(typ))
    return before, x


def test_minp_one_keeps_exactly_the_legal_maxima():
    _, x = _apply([[1.0, 3.0, 2.0, 3.0, -1.0, 9.0]], [0, 1, 2, 3, 4], [1.0], [1.0])
    assert x[0].tolist() == [NEG, 3.0, NEG, 3.0, NEG, 9.0]  # token 5 is illegal: ignored and left untouched


def test_neutral_parameters_change_nothing():
    before, x = _apply([[1.0, 3.0, 2.0, 3.0, -1.0, 9.0]], [0, 1, 2, 3, 4], [0.0], [1.0])
    assert torch.equal(before, x)


def test_minp_threshold_is_relative_to_the_maximum():
    # ln 0.5 = -0.693: survivors are x >= 3 - 0.693
    _, x = _apply([[2.5, 3.0, 2.25, 2.3125, NEG]], [0, 1, 2, 3, 4], [0.5], [1.0])
    assert x[0].tolist() == [2.5, 3.0, NEG, 2.3125, NEG]


def test_typical_removes_the_most_probable_token_and_minp_keys_off_the_survivors():
    # p = (0.4, 0.15 x 4): H = 1.505 nats; -log p = 0.916 for the head (d = 0.588) and 1.897 for the tail (d = 0.392).
    # The tail class comes first and already carries 0.6 > 0.4: it is the boundary, the head is removed.
    head, tail = (float(torch.tensor(math.log(p))) for p in (0.4, 0.15))  # as fp32 holds them
    row = [head, tail, tail, tail, tail, 7.0]
    _, x = _apply([row], [0, 1, 2, 3, 4], [0.0], [0.4])
    assert x[0].tolist() == [NEG] + row[1:]
    # min_p = 0.9 after it: the survivors' maximum is the tail value itself (the removed head would have cut them all)
    _, y = _apply([row], [0, 1, 2, 3, 4], [0.9], [0.4])
    assert y[0].tolist() == [NEG] + row[1:]
    _, z = _apply([row], [0, 1, 2, 3, 4], [0.9], [1.0])
    assert z[0].tolist() == [head, NEG, NEG, NEG, NEG, 7.0]
    # typical_p above the tail's mass: the boundary moves on to the head, everything survives
    before, w = _apply([row], [0, 1, 2, 3, 4], [0.0], [0.7])
    assert torch.equal(before, w)


def test_equal_logits_share_their_fate():
    row = [0.0, 0.0, 0.0, 1.5, 1.5, -2.0, -2.0, -2.0]
    for tp in (0.05, 0.3, 0.6, 0.9, 0.99):
        _, x = _apply([row], list(range(8)), [0.0], [tp])
        kept = [v > NEG for v in x[0].tolist()]
        assert any(kept)
        for grp in ((0, 1, 2), (3, 4), (5, 6, 7)):
            assert len({kept[i] for i in grp}) == 1, (tp, kept)


def test_single_legal_token_and_all_neginf_rows_are_untouched():
    before, x = _apply([[1.0, 5.0, 2.0], [NEG, NEG, 4.0]], [1], [1.0, 1.0], [0.2, 0.2])
    assert torch.equal(before, x)  # one legal token: a grammar-forced token stays forced
    before, x = _apply([[NEG, NEG, 4.0]], [0, 1], [1.0], [0.2])
    assert torch.equal(before, x)  # no legal logit above -inf


def test_dead_unsampled_and_greedy_slots_are_untouched():
    row = [1.0, 3.0, 2.0, 0.5]
    before, x = _apply([row] * 5, [0, 1, 2, 3], [1.0] * 5, [0.5] * 5, state=[DONE, -3, -1, 1, 1],
                       row_of_slot=[0, 1, 2, -1, 4], temp=[1.0, 1.0, 1.0, 1.0, 0.0])
    assert torch.equal(before, x)
    _, y = _apply([row] * 2, [0, 1, 2, 3], [1.0] * 2, [1.0] * 2, row_of_slot=[1, -1])
    assert y.tolist() == [row, [NEG, 3.0, NEG, NEG]]  # slot 0 rewrote logits row 1


def test_survivor_helper_matches_the_op():
    g = torch.Generator().manual_seed(3)
    nxt, dist = tc.build_dfa(1003, g)
    legal = tc.legal_mask(nxt, dist, tc.ST_GEN, tc.REMAINING)
    x = torch.randn(1003, generator=g) * 2
    keep = ops.truncate_survivors(x, legal, math.log(0.1), 0.7)
    y = x.clone()[None]
    ops.truncate_logits(y, None, nxt, dist, DONE, torch.tensor([tc.ST_GEN], dtype=torch.int32),
                        torch.tensor([tc.REMAINING], dtype=torch.int32), torch.ones(1), torch.tensor([math.log(0.1)]),
                        torch.tensor([0.7]))
    assert torch.equal(y[0] > NEG, keep | ~legal) and torch.equal(y[0][keep | ~legal], x[keep | ~legal])
    assert 0 < int(keep.sum()) < int(legal.sum())


@pytest.mark.parametrize("vocab", [1003, 128256])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_shared_cases_on_the_reference_path(vocab, dt):
    tc.check_minp(3, vocab, dt, "cpu")
    tc.check_minp(64, vocab, dt, "cpu")
    tc.check_typical_ladder(vocab, dt, "cpu", False)
    tc.check_typical_ladder(vocab, dt, "cpu", True)


def test_random_rows_and_sampler_on_the_reference_path():
    tc.check_typical_random("bf16", "cpu", 0.5, seed=1)
    tc.check_sampler_after("cpu")


# ---- protocol -------------------------------------------------------------------------------------------------------
def test_options_parse_and_default_to_neutral():
    p = GenerateParams.parse({"prompt": "x", "options": {"temperature": 0.8, "min_p": 0.05, "typical_p": 0.9}})
    assert (p.min_p, p.typical_p) == (0.05, 0.9)
    d = GenerateParams.parse({"prompt": "x", "options": {"temperature": 0.8}})
    assert (d.min_p, d.typical_p, d.unsupported) == (0.0, 1.0, ())
    e = GenerateParams.parse({"prompt": "x", "options": {"min_p": 1, "typical_p": 1}})
    assert (e.min_p, e.typical_p) == (1.0, 1.0)
    assert GenerateParams.parse({"prompt": "x", "options": {"min_p": 0}}).min_p == 0.0


@pytest.mark.parametrize("opts,name", [
    ({"min_p": -0.1}, "min_p"), ({"min_p": 1.5}, "min_p"), ({"min_p": "0.05"}, "min_p"), ({"min_p": True}, "min_p"),
    ({"min_p": float("nan")}, "min_p"), ({"min_p": float("inf")}, "min_p"), ({"min_p": None}, "min_p"),
    ({"typical_p": 0}, "typical_p"), ({"typical_p": -1}, "typical_p"), ({"typical_p": 1.01}, "typical_p"),
    ({"typical_p": "1"}, "typical_p"), ({"typical_p": False}, "typical_p"), ({"typical_p": float("nan")}, "typical_p"),
    ({"typical_p": [0.5]}, "typical_p")])
def test_bad_options_are_400(opts, name):
    for chat in (False, True):
        with pytest.raises(BadRequest, match=name):
            GenerateParams.parse({"prompt": "x", "messages": [{"role": "user", "content": "x"}], "options": opts},
                                 chat=chat)


def test_bad_option_is_a_400_over_http():
    from chronos.brain.api.server import FakeBackend
    from test_api import Server

    s = Server(FakeBackend("ok"))
    try:
        r = requests.post(f"{s.url}/api/generate", timeout=10,
                          json={"prompt": "x", "stream": False, "options": {"min_p": 2}})
        assert r.status_code == 400 and "min_p" in r.json()["error"]
        r = requests.post(f"{s.url}/api/chat", timeout=10, json={"messages": [{"role": "user", "content": "x"}],
                                                                  "stream": False, "options": {"typical_p": 0}})
        assert r.status_code == 400 and "typical_p" in r.json()["error"]
    finally:
        s.close()


def test_mirostat_and_tfs_z_are_named_on_every_backend():
    from types import SimpleNamespace

    def named(opts, req):
        return penalties_ignored(GenerateParams.parse({"prompt": "x", "options": opts}), req)

    engine_req = SimpleNamespace(penalty=None, truncates=False)
    fake_req = SimpleNamespace()
    for req in (engine_req, fake_req):
        assert named({"mirostat": 2, "mirostat_tau": 5.0, "mirostat_eta": 0.1}, req) == \
            ("mirostat", "mirostat_tau", "mirostat_eta")
        assert named({"mirostat": 1}, req) == ("mirostat",)
        assert named({"mirostat": 0, "mirostat_tau": 5.0, "mirostat_eta": 0.1}, req) == ()
        assert named({"mirostat_tau": 5.0}, req) == ()
        assert named({"tfs_z": 0.95}, req) == ("tfs_z",)
        assert named({"tfs_z": 1}, req) == () and named({"tfs_z": 1.0}, req) == ()
        assert named({}, req) == ()


def test_fake_backend_names_the_options_and_the_engine_backend_does_not():
    from chronos.brain.api.server import FakeBackend
    from chronos.brain.api.service import EngineService
    from chronos.brain.engine.engine import EngineConfig
    from test_api import Server

    def gen(s, opts):
        r = requests.post(f"{s.url}/api/generate", timeout=120,
                          json={"prompt": "tell me", "stream": False, "options": dict({"num_predict": 10}, **opts)})
        assert r.status_code == 200, r.text
        return r.json()

    def stream(s, opts):
        r = requests.post(f"{s.url}/api/generate", stream=True, timeout=120,
                          json={"prompt": "tell me", "options": dict({"num_predict": 10}, **opts)})
        return [json.loads(l) for l in r.iter_lines() if l][-1]

    both = {"temperature": 0.8, "seed": 4, "min_p": 0.5, "typical_p": 0.7}
    s = Server(FakeBackend("ok"))
    try:
        assert gen(s, both)["ignored_options"] == ["min_p", "typical_p"]
        assert gen(s, dict(both, typical_p=1.0))["ignored_options"] == ["min_p"]
        assert gen(s, dict(both, min_p=0))["ignored_options"] == ["typical_p"]
        assert "ignored_options" not in gen(s, {"temperature": 0.8, "min_p": 0.0, "typical_p": 1})
        assert stream(s, both)["ignored_options"] == ["min_p", "typical_p"]
        assert gen(s, dict(both, tfs_z=0.9, repeat_penalty=1.2))["ignored_options"] == \
            ["repeat_penalty", "min_p", "typical_p", "tfs_z"]
    finally:
        s.close()
    svc = EngineService.from_config(EngineConfig(model="tiny", device="cpu", max_slots=4, max_model_len=384,
                                                 use_graphs=False, decode_burst=4))
    s = Server(svc)
    try:
        plain = gen(s, {"temperature": 0.8, "seed": 4})
        cut = gen(s, dict(both, min_p=1.0))
        assert "ignored_options" not in cut and "ignored_options" not in plain
        assert cut["response"] != plain["response"], "min_p = 1 on a sampled request changes what is drawn"
        assert "ignored_options" not in stream(s, both)
        assert gen(s, dict(both, mirostat=1))["ignored_options"] == ["mirostat"]
        assert svc.engine.stats["truncate_launches"] > 0
    finally:
        s.close()
        svc.close()


# ---- engine, tiny model ---------------------------------------------------------------------------------------------
def test_engine_minp_one_picks_a_maximal_legal_logit_at_every_step(monkeypatch):
    te.check_minp1("cpu", monkeypatch)


def test_engine_mixed_batch_leaves_the_other_requests_token_identical(monkeypatch):
    te.check_mixed("cpu", monkeypatch)


def test_engine_never_asked_launches_nothing_and_keeps_its_graph_keys():
    te.check_never_asked("cpu")


def test_engine_slot_reuse_resets_the_parameters():
    te.check_slot_reuse("cpu")


def test_graph_key_variants():
    from chronos.brain.engine.engine import Engine

    assert Engine._gkey(8, 1, 4, False, False) == (8, 1, 4)
    assert Engine._gkey(8, 1, 4, True, False) == (8, 1, 4, 1)
    assert Engine._gkey(8, 1, 4, True, True) == (8, 1, 4, 1, "pen")
    assert Engine._gkey(8, 1, 4, False, False, True) == (8, 1, 4, 0, 0, "tr")
    assert Engine._gkey(8, 1, 4, True, True, True) == (8, 1, 4, 1, 1, "tr")
