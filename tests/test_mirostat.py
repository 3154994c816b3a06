"""Mirostat 2.0 on the CPU: ops.reference against the fp64 oracle on the shared cases of tests/_mirostat_cases.py,
mutations of the computation caught at twice the margins, the API options (400s, ``ignored_options``), and the engine
on the tiny model with the checks of tests/_mirostat_engine.py."""
import json
import os
import sys

import pytest
import requests
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mirostat_cases as mc  # noqa: E402
import _mirostat_engine as me  # noqa: E402

from chronos import ops  # noqa: E402
from chronos.brain.api.protocol import BadRequest, GenerateParams, penalties_ignored  # noqa: E402

DEV = "cpu"


# ---- the reference against the oracle -------------------------------------------------------------------------------
def test_reference_on_the_shared_cases():
    mc.check_all(DEV)


def test_ladder_case_covers_every_kind_of_slot():
    c = mc.ladder_case(1003, "bf16")
    kinds = [sp["kind"] for sp in c.slots]
    assert {"live", "done", "parked", "empty", "norow"} <= set(kinds)
    active = [s for s in range(c.n) if c.active(s)]
    assert active == [0, 7, 8, 11, 12]  # greedy (5), off (6), one legal token (9), all -inf (10) are left alone
    res = mc.check(c, DEV)
    kept = lambda s: int((c.legal(s) & (res["buf"][c.perm[s], :c.vocab].float() > mc.NEG)).sum())  # noqa: E731
    assert kept(7) == 2, "mu below every surprise: the two tied maxima survive"
    assert kept(8) == int(c.legal(8).sum()), "mu above every surprise: nothing is removed"
    assert 2 < kept(0) < int(c.legal(0).sum())
    for s in (1, 2, 3):  # NaN rows of skipped slots come back bit for bit (violations() compares the whole buffer)
        assert bool(torch.isnan(res["buf"][c.perm[s], :c.vocab].float()).all())


def test_row_helper_matches_the_op():
    c = mc.ladder_case(1003, "f32")
    res = c.run(DEV)
    keep, m, lnz = ops.mirostat_row(c.x(0), c.legal(0), 0.5, float(c.mu[0]))
    assert torch.equal(keep, c.legal(0) & (res["buf"][c.perm[0], :c.vocab] > mc.NEG))
    assert float(m) == float(res["m"][0]) and float(lnz) == float(res["lnz"][0])
    assert ops.mirostat_row(c.x(9), c.legal(9), 1.0, 0.5) is None and ops.mirostat_row(c.x(10), c.legal(10), 1.0, 0.5) \
        is None


def test_the_fp64_impostor_passes_its_own_checks():
    for c in (mc.ladder_case(1003, "f32"), mc.random_case(1003, "bf16", 0.5, "perm", seed=1)):
        t, u = mc.impostor(c, None)
        assert c.violations(c.run(DEV, truncate=t, update=u)) == []


@pytest.mark.parametrize("mut", mc.MUTATIONS)
def test_mutations_land_twice_outside_the_bounds(mut):
    """Each wrong variant, computed in fp64, violates the checks at twice the margins on the slots where it applies."""
    c = mc.ladder_case(1003, "f32")
    t, u = mc.impostor(c, mut)
    bad = c.violations(c.run(DEV, truncate=t, update=u), scale=2.0)
    hit = {int(b.split(" slot ")[1].split(":")[0]) for b in bad if " slot " in b}
    applies = {"mu_frozen": {0, 7, 8, 11, 12}, "z_for_zprime": {0, 7, 11, 12}, "nats": {0, 7, 8, 11, 12},
               "no_T": {0, 11}, "forced_moves": {9, 10}, "swap": {0, 7, 8, 11, 12}}[mut]
    print(mut, sorted(hit), bad[:4])
    assert applies <= hit, (mut, sorted(applies - hit), bad)


# ---- protocol -------------------------------------------------------------------------------------------------------
def _parse(opts, chat=False):
    return GenerateParams.parse({"prompt": "x", "messages": [{"role": "user", "content": "x"}], "options": opts},
                                chat=chat)


def test_options_parse_and_default():
    p = _parse({"temperature": 0.8, "mirostat": 2})
    assert (p.mirostat, p.mirostat_tau, p.mirostat_eta, p.unsupported) == (2, 5.0, 0.1, ())
    p = _parse({"temperature": 0.8, "mirostat": 2, "mirostat_tau": 3, "mirostat_eta": 0})
    assert (p.mirostat, p.mirostat_tau, p.mirostat_eta) == (2, 3.0, 0.0)
    assert _parse({}).mirostat == 0 and _parse({"mirostat": 0, "mirostat_tau": -1}).mirostat == 0
    for other in (1, 3, 2.5, True, "2"):  # today's behaviour, lack of validation included
        q = _parse({"mirostat": other, "mirostat_tau": "x"})
        assert q.mirostat == 0 and q.unsupported == ("mirostat", "mirostat_tau")


@pytest.mark.parametrize("opts,name", [
    ({"mirostat_tau": -0.1}, "mirostat_tau"), ({"mirostat_tau": "5"}, "mirostat_tau"),
    ({"mirostat_tau": None}, "mirostat_tau"), ({"mirostat_tau": float("nan")}, "mirostat_tau"),
    ({"mirostat_tau": float("inf")}, "mirostat_tau"), ({"mirostat_tau": True}, "mirostat_tau"),
    ({"mirostat_eta": -1}, "mirostat_eta"), ({"mirostat_eta": "0.1"}, "mirostat_eta"),
    ({"mirostat_eta": [0.1]}, "mirostat_eta"), ({"mirostat_eta": float("nan")}, "mirostat_eta")])
def test_bad_options_are_400(opts, name):
    for chat in (False, True):
        with pytest.raises(BadRequest, match=name):
            _parse(dict(opts, mirostat=2), chat=chat)


def test_ignored_options_by_request_object():
    from types import SimpleNamespace

    def named(opts, req):
        return penalties_ignored(_parse(opts), req)

    three = {"mirostat": 2, "mirostat_tau": 5.0, "mirostat_eta": 0.1}
    all3 = ("mirostat", "mirostat_tau", "mirostat_eta")
    applied = SimpleNamespace(penalty=None, truncates=False, mirostat=True)
    declined = SimpleNamespace(penalty=None, truncates=False, mirostat=False)
    fake = SimpleNamespace()
    assert named(dict(three, temperature=0.8), applied) == ()
    assert named(dict(three, temperature=0.8), declined) == all3
    assert named(dict(three, temperature=0.8), fake) == all3
    assert named(three, declined) == (), "temperature 0: greedy, nothing is named"
    assert named({"mirostat": 2, "temperature": 0.8}, fake) == ("mirostat",)
    assert named({"mirostat": 2, "temperature": 0.8, "tfs_z": 0.9}, fake) == ("mirostat", "tfs_z")
    assert named({"mirostat": 1, "temperature": 0.8}, applied) == ("mirostat",)


def test_fake_backend_names_the_options_and_the_engine_backend_does_not():
    from chronos.brain.api.server import FakeBackend
    from chronos.brain.api.service import EngineService
    from chronos.brain.engine.engine import EngineConfig
    from test_api import Server

    def gen(s, opts, expect=200):
        r = requests.post(f"{s.url}/api/generate", timeout=120,
                          json={"prompt": "tell me", "stream": False, "options": dict({"num_predict": 10}, **opts)})
        assert r.status_code == expect, r.text
        return r.json()

    def stream(s, opts):
        r = requests.post(f"{s.url}/api/generate", stream=True, timeout=120,
                          json={"prompt": "tell me", "options": dict({"num_predict": 10}, **opts)})
        return [json.loads(l) for l in r.iter_lines() if l][-1]

    on = {"temperature": 0.8, "seed": 4, "mirostat": 2, "mirostat_tau": 1.0, "mirostat_eta": 0.3}
    s = Server(FakeBackend("ok"))
    try:
        assert gen(s, on)["ignored_options"] == ["mirostat", "mirostat_tau", "mirostat_eta"]
        assert stream(s, on)["ignored_options"] == ["mirostat", "mirostat_tau", "mirostat_eta"]
        assert "mirostat_tau" in gen(s, dict(on, mirostat_tau=-1), expect=400)["error"]
        r = requests.post(f"{s.url}/api/chat", timeout=10, json={
            "messages": [{"role": "user", "content": "x"}], "stream": False, "options": dict(on, mirostat_eta="a")})
        assert r.status_code == 400 and "mirostat_eta" in r.json()["error"]
    finally:
        s.close()
    svc = EngineService.from_config(EngineConfig(model="tiny", device="cpu", max_slots=4, max_model_len=384,
                                                 use_graphs=False, decode_burst=4))
    s = Server(svc)
    try:
        greedy = gen(s, dict(on, temperature=0))
        assert "ignored_options" not in greedy and svc.engine.stats["mirostat_launches"] == 0
        assert svc.engine.s_mion is None, "mirostat at temperature 0 allocates nothing"
        plain = gen(s, {"temperature": 0.8, "seed": 4})
        cut = gen(s, on)
        assert "ignored_options" not in cut and "ignored_options" not in plain
        assert svc.engine.stats["mirostat_launches"] > 0
        assert cut["response"] != plain["response"], "tau = 1 on a sampled request changes what is drawn"
        assert "ignored_options" not in stream(s, on)
        assert "ignored_options" not in gen(s, dict(on, top_k=5, top_p=0.5, min_p=0.3))
        assert gen(s, dict(on, mirostat=1))["ignored_options"] == ["mirostat", "mirostat_tau", "mirostat_eta"]
    finally:
        s.close()
        svc.close()


# ---- engine, tiny model ---------------------------------------------------------------------------------------------
def test_engine_submit_arguments():
    eng = me.engine(DEV, max_slots=2)
    r = eng.submit([1, 2, 3], num_predict=2, temperature=0.9, top_k=5, top_p=0.5, min_p=0.2, typical_p=0.5, mirostat=2,
                   mirostat_tau=3.0, mirostat_eta=0.2)
    assert r.mirostat and (r.mirostat_tau, r.mirostat_eta, r.mirostat_mu) == (3.0, 0.2, 6.0)
    assert (r.top_k, r.top_p, r.min_p, r.typical_p) == (0, 1.0, 0.0, 1.0) and not r.truncates
    d = eng.submit([1, 2, 3], num_predict=2, temperature=0.9, mirostat=2)
    assert d.mirostat and (d.mirostat_tau, d.mirostat_eta, d.mirostat_mu) == (5.0, 0.1, 10.0)
    g = eng.submit([1, 2, 3], num_predict=2, temperature=0.0, top_k=5, min_p=0.2, mirostat=2)
    assert not g.mirostat and g.top_k == 5
    for other in (0, 1, 3, True, None):
        o = eng.submit([1, 2, 3], num_predict=2, temperature=0.9, min_p=0.2, mirostat=other)
        assert not o.mirostat and o.min_p == 0.2 and o.truncates


def test_engine_trajectory_replayed_from_logprobs():
    me.check_trajectory(DEV)


def test_engine_jump_forward_leaves_mu_alone(monkeypatch):
    me.check_jump_forward(DEV, monkeypatch)


def test_engine_preemption_resumes_from_the_saved_mu(monkeypatch):
    me.check_preemption(DEV, monkeypatch)


def test_engine_slot_reuse_resets_flag_and_mu(monkeypatch):
    me.check_slot_reuse(DEV, monkeypatch)


def test_engine_never_asked_allocates_nothing_and_keeps_its_graph_keys():
    me.check_never_asked(DEV)


def test_engine_mixed_batch_leaves_the_other_requests_token_identical():
    me.check_mixed(DEV)


def test_graph_key_variants():
    from chronos.brain.engine.engine import Engine

    assert Engine._gkey(8, 1, 4, False, False) == (8, 1, 4)
    assert Engine._gkey(8, 1, 4, True, False) == (8, 1, 4, 1)
    assert Engine._gkey(8, 1, 4, True, True) == (8, 1, 4, 1, "pen")
    assert Engine._gkey(8, 1, 4, False, True, True) == (8, 1, 4, 0, 1, "tr")
    assert Engine._gkey(8, 1, 4, False, False, False, True) == (8, 1, 4, 0, 0, 0, "mi")
    assert Engine._gkey(8, 1, 4, True, True, True, True) == (8, 1, 4, 1, 1, 1, "mi")
