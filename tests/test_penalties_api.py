"""``options.repeat_penalty`` / ``frequency_penalty`` / ``presence_penalty`` / ``repeat_last_n`` through the REST API
(brain/api/protocol.py) and the DP router: the 400s, a penalised reply that differs from the unpenalised one and is
still valid schema JSON, ``ignored_options`` only from backends that cannot apply them, ``repeat_last_n: 0``."""
import asyncio
import json

import pytest
import requests

from chronos.brain.api.server import FakeBackend
from test_api import Server

CHAIN = ["[OPEN] attack_chain.sh -> /tmp/malware.bin", "[EXEC] attack_chain.sh -> curl"]
PROMPT = "tell me"  # the tiny random model repeats itself on it (asserted below), so a repeat penalty changes the reply
PEN = {"repeat_penalty": 1.3}


def _cfg(**kw):
    from chronos.brain.engine.engine import EngineConfig

    base = dict(model="tiny", device="cpu", max_slots=4, max_model_len=384, use_graphs=False, decode_burst=4)
    base.update(kw)
    return EngineConfig(**base)


@pytest.fixture(scope="module")
def service():
    from chronos.brain.api.service import EngineService

    svc = EngineService.from_config(_cfg(penalty_window=64))
    s = Server(svc)
    yield s
    s.close()
    svc.close()


@pytest.fixture(scope="module")
def plain_service():
    """The default EngineConfig: penalty_window 0, penalties accepted and not applied."""
    from chronos.brain.api.service import EngineService

    svc = EngineService.from_config(_cfg())
    s = Server(svc)
    yield s
    s.close()
    svc.close()


def _gen(s, opts, **body):
    r = requests.post(f"{s.url}/api/generate", timeout=120,
                      json=dict({"prompt": PROMPT, "stream": False}, options=dict({"num_predict": 16}, **opts), **body))
    assert r.status_code == 200, r.text
    return r.json()


def _chat(s, opts, **body):
    r = requests.post(f"{s.url}/api/chat", timeout=120,
                      json=dict({"messages": [{"role": "user", "content": PROMPT}], "stream": False},
                                options=dict({"num_predict": 16}, **opts), **body))
    assert r.status_code == 200, r.text
    return r.json()


def _stream(s, opts):
    r = requests.post(f"{s.url}/api/generate", stream=True, timeout=120,
                      json={"prompt": PROMPT, "options": dict({"num_predict": 16}, **opts)})
    lines = [json.loads(l) for l in r.iter_lines() if l]
    assert lines[-1]["done"]
    return "".join(l["response"] for l in lines), lines[-1]


@pytest.mark.parametrize("opts,name", [
    ({"repeat_penalty": 0}, "repeat_penalty"), ({"repeat_penalty": -1.5}, "repeat_penalty"),
    ({"repeat_penalty": "1.1"}, "repeat_penalty"), ({"repeat_penalty": True}, "repeat_penalty"),
    ({"repeat_penalty": float("inf")}, "repeat_penalty"), ({"repeat_penalty": None}, "repeat_penalty"),
    ({"frequency_penalty": "x"}, "frequency_penalty"), ({"frequency_penalty": float("nan")}, "frequency_penalty"),
    ({"presence_penalty": [1]}, "presence_penalty"), ({"presence_penalty": float("-inf")}, "presence_penalty"),
    ({"repeat_last_n": -2}, "repeat_last_n"), ({"repeat_last_n": 1.5}, "repeat_last_n"),
    ({"repeat_last_n": "64"}, "repeat_last_n"), ({"repeat_last_n": False}, "repeat_last_n")])
def test_bad_penalty_options_are_400(opts, name):
    s = Server(FakeBackend("ok"))
    try:
        # (json.dumps writes Infinity / NaN as bare words, which the server's parser reads back as floats)
        r = requests.post(f"{s.url}/api/generate", timeout=10, headers={"Content-Type": "application/json"},
                          data=json.dumps({"prompt": "x", "stream": False, "options": opts}))
        assert r.status_code == 400 and name in r.json()["error"], r.text
        r = requests.post(f"{s.url}/api/chat", timeout=10, headers={"Content-Type": "application/json"},
                          data=json.dumps({"messages": [{"role": "user", "content": "x"}], "stream": False,
                                           "options": opts}))
        assert r.status_code == 400 and name in r.json()["error"], r.text
    finally:
        s.close()


def test_valid_penalty_options_parse():
    from chronos.brain.api.protocol import GenerateParams

    p = GenerateParams.parse({"prompt": "x", "options": {"repeat_penalty": 2, "frequency_penalty": -0.5,
                                                         "presence_penalty": 0.25, "repeat_last_n": -1}})
    assert (p.repeat_penalty, p.frequency_penalty, p.presence_penalty, p.repeat_last_n) == (2.0, -0.5, 0.25, -1)
    assert p.ignored == ("repeat_penalty", "frequency_penalty", "presence_penalty")
    d = GenerateParams.parse({"prompt": "x"})
    assert (d.repeat_penalty, d.frequency_penalty, d.presence_penalty, d.repeat_last_n) == (1.0, 0.0, 0.0, 64)
    assert d.ignored == ()
    assert GenerateParams.parse({"prompt": "x", "options": {"repeat_penalty": 1.3, "repeat_last_n": 0}}).ignored == ()
    assert GenerateParams.parse({"prompt": "x", "options": {"repeat_penalty": 1.0, "presence_penalty": 0}}).ignored == ()


def test_engine_applies_penalties_generate_chat_stream(service, plain_service):
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    base = _gen(service, {})
    ids = base["context"][-base["eval_count"]:]
    assert len(set(ids)) < len(ids), "the prompt was chosen so that the unpenalised reply repeats a token"
    pen = _gen(service, PEN)
    assert "ignored_options" not in pen and pen["response"] != base["response"]
    assert _gen(plain_service, {})["response"] == base["response"]
    # repeat_last_n 0 switches the penalties off for the request: the unpenalised text, nothing ignored
    off = _gen(service, dict(PEN, repeat_last_n=0))
    assert off["response"] == base["response"] and "ignored_options" not in off
    # chat
    cbase, cpen = _chat(service, {}), _chat(service, PEN)
    assert "ignored_options" not in cpen and cpen["message"]["content"] != cbase["message"]["content"]
    coff = _chat(service, dict(PEN, repeat_last_n=0))
    assert coff["message"]["content"] == cbase["message"]["content"] and "ignored_options" not in coff
    # stream
    text, last = _stream(service, PEN)
    assert text == pen["response"] and "ignored_options" not in last
    text, last = _stream(service, dict(PEN, repeat_last_n=0))
    assert text == base["response"] and "ignored_options" not in last
    # with a format the penalised reply is still valid schema JSON
    v = _gen(service, dict(PEN, presence_penalty=1.0, num_predict=60), prompt=build_prompt(CHAIN), format=VERDICT_SCHEMA)
    verdict = json.loads(v["response"])
    assert set(verdict) == {"risk_score", "verdict", "reason"} and "ignored_options" not in v
    assert isinstance(verdict["risk_score"], int) and verdict["verdict"] in ("SAFE", "SUSPICIOUS", "MALICIOUS")
    assert service.backend.engine.stats["penalty_launches"] > 0
    assert plain_service.backend.engine.stats["penalty_launches"] == 0


def test_backends_that_cannot_name_the_option_and_answer_unpenalised(plain_service):
    base = _gen(plain_service, {})
    pen = _gen(plain_service, PEN)
    assert pen["ignored_options"] == ["repeat_penalty"] and pen["response"] == base["response"]
    both = _gen(plain_service, {"frequency_penalty": 0.5, "presence_penalty": -0.5, "repeat_penalty": 1.0})
    assert both["ignored_options"] == ["frequency_penalty", "presence_penalty"] and both["response"] == base["response"]
    off = _gen(plain_service, dict(PEN, repeat_last_n=0))
    assert "ignored_options" not in off and off["response"] == base["response"]
    cbase, cpen = _chat(plain_service, {}), _chat(plain_service, PEN)
    assert cpen["ignored_options"] == ["repeat_penalty"]
    assert cpen["message"]["content"] == cbase["message"]["content"]
    text, last = _stream(plain_service, PEN)
    assert last["ignored_options"] == ["repeat_penalty"] and text == base["response"]
    s = Server(FakeBackend("ok"))
    try:
        b = _gen(s, PEN)
        assert b["ignored_options"] == ["repeat_penalty"] and b["response"] == _gen(s, {})["response"]
        assert _chat(s, PEN)["ignored_options"] == ["repeat_penalty"]
        assert _stream(s, PEN)[1]["ignored_options"] == ["repeat_penalty"]
        assert "ignored_options" not in _gen(s, dict(PEN, repeat_last_n=0))
        assert "ignored_options" not in _gen(s, {}) and "ignored_options" not in _chat(s, {})
    finally:
        s.close()


def test_dp_router_passes_penalties_through():
    from chronos.brain.api.protocol import GenerateParams, penalties_ignored
    from chronos.parallel.router import DPRouter

    router = DPRouter(_cfg(penalty_window=64), 1)
    try:
        async def go():
            ps = [GenerateParams.parse({"prompt": PROMPT, "stream": False, "options": dict({"num_predict": 16}, **o)})
                  for o in ({}, PEN, dict(PEN, repeat_last_n=0))]
            return ps, await asyncio.gather(*[router.generate(p) for p in ps])

        ps, (base, pen, off) = asyncio.run(go())
        assert pen.penalty == (1.3, 0.0, 0.0, 64) and base.penalty is None and off.penalty is None
        assert pen.out_ids != base.out_ids and off.out_ids == base.out_ids
        assert [penalties_ignored(p, r) for p, r in zip(ps, (base, pen, off))] == [(), (), ()]
    finally:
        router.close()
