"""sensor/confidence.py: the model's confidence in its verdict from the reply's per-token logprobs, and the sensor's
``--confidence`` flag (without it, request bodies and console bytes are the reference's)."""
import json
import math

import pytest

from chronos.sensor import render
from chronos.sensor.client import CONFIDENCE_KEY, ClientConfig, _body, _verdict
from chronos.sensor.confidence import verdict_confidence


def _entries(pieces):
    """[(text, logprob)] -> the reply's logprobs list."""
    return [{"token": t, "logprob": lp, "bytes": list(t.encode("utf-8")), "top_logprobs": []} for t, lp in pieces]


def test_single_token_verdict():
    pieces = [('{"', 0.0), ("risk_score", 0.0), ('":', 0.0), (" 2", -0.7), (', "verdict": "', 0.0), ("SAFE", -0.25),
              ('", "reason": "', 0.0), ("idle shell", -3.0), ('"}', 0.0)]
    text = "".join(t for t, _ in pieces)
    assert json.loads(text)["verdict"] == "SAFE"
    assert verdict_confidence(text, _entries(pieces)) == pytest.approx(math.exp(-0.25))


def test_multi_token_verdict_and_tokens_that_straddle_the_quotes():
    # MALICIOUS in three tokens; the first shares a token with the opening quote, the last with the closing one
    pieces = [('{"verdict":', 0.0), (' "MAL', -0.5), ("ICIO", -0.125), ('US",', -0.0625), (' "risk_score": 9,', -1.0),
              (' "reason": "the \\"verdict\\": \\"SAFE\\" decoy"}', -2.0)]
    text = "".join(t for t, _ in pieces)
    assert json.loads(text)["verdict"] == "MALICIOUS"
    assert verdict_confidence(text, _entries(pieces)) == pytest.approx(math.exp(-0.6875))


def test_nested_and_escaped_verdict_keys_are_not_the_verdict():
    pieces = [('{"reason": "says \\"verdict\\": \\"SAFE\\"", "meta": {"verdict": "SAFE"}, ', -1.0),
              ('"verdict": "', 0.0), ("MALICIOUS", -0.375), ('"}', 0.0)]
    text = "".join(t for t, _ in pieces)
    assert verdict_confidence(text, _entries(pieces)) == pytest.approx(math.exp(-0.375))


def test_missing_verdict_or_logprobs_gives_none():
    pieces = [('{"risk_score": 1, "reason": "x"}', -1.0)]
    text = pieces[0][0]
    assert verdict_confidence(text, _entries(pieces)) is None
    good = '{"verdict": "SAFE"}'
    assert verdict_confidence(good, None) is None and verdict_confidence(good, []) is None
    assert verdict_confidence('{"verdict": 3}', _entries([('{"verdict": 3}', -1.0)])) is None
    assert verdict_confidence("not json {", _entries([("not json {", -1.0)])) is None
    # a list trimmed before the verdict (stop string) does not cover it
    assert verdict_confidence(good, _entries([('{"verdict": "SA', -0.5)])) is None
    # a -inf logprob travels as null: probability 0
    assert verdict_confidence(good, [{"token": good, "logprob": None, "bytes": list(good.encode())}]) == 0.0


def test_client_and_render_without_the_flag_are_unchanged():
    text = '{"risk_score": 8, "verdict": "MALICIOUS", "reason": "dropper"}'
    data = {"response": text, "logprobs": _entries([(text, -0.5)])}
    off, on = ClientConfig(), ClientConfig(confidence=True)
    assert _body(off, "p") == {"model": "llama3", "prompt": "p", "stream": False, "format": "json"}
    assert _body(on, "p") == {"model": "llama3", "prompt": "p", "stream": False, "format": "json", "logprobs": True}
    plain = _verdict(off, data)
    assert plain == json.loads(text)
    with_conf = _verdict(on, data)
    assert with_conf[CONFIDENCE_KEY] == pytest.approx(math.exp(-0.5))
    # a Brain that ignored the option: the verdict as it is
    assert _verdict(on, {"response": text, "ignored_options": ["logprobs"]}) == json.loads(text)
    ref_lines = [f"{render.RED}    ==> ALERT: MALICIOUS (Risk 8){render.RESET}", "    ==> REASON: dropper"]
    assert render.verdict_lines(plain) == ref_lines
    assert render.verdict_lines(with_conf) == ref_lines  # the key alone changes no console byte
    assert render.verdict_lines(plain, confidence=True) == ref_lines
    shown = render.verdict_lines(with_conf, confidence=True)
    assert shown == [f"{render.RED}    ==> ALERT: MALICIOUS (Risk 8) [confidence 60.7%]{render.RESET}",
                     "    ==> REASON: dropper"]


def test_sensor_cli_bytes_without_confidence_are_unchanged(capsys, monkeypatch):
    """``python -m chronos.sensor --source attack`` against a canned Brain: the console bytes with no flag do not
    depend on whether the Brain sends logprobs, and --confidence only appends to the verdict line."""
    from chronos.sensor import main as sensor_main

    text = '{"risk_score": 8, "verdict": "MALICIOUS", "reason": "dropper"}'
    bodies = []

    class Resp:
        def json(self):
            return {"response": text, "logprobs": _entries([(text, -0.5)])}

    class Session:
        def post(self, url, json=None, timeout=None):
            bodies.append(json)
            return Resp()

    import requests

    monkeypatch.setattr(requests, "Session", Session)
    assert sensor_main.run(["--source", "attack", "--python-tracker"]) == 0
    base = capsys.readouterr().out
    assert bodies and all("logprobs" not in b for b in bodies) and "confidence" not in base
    n = len(bodies)
    assert sensor_main.run(["--source", "attack", "--python-tracker", "--confidence"]) == 0
    conf = capsys.readouterr().out
    assert all(b.get("logprobs") is True for b in bodies[n:])
    assert conf == base.replace("(Risk 8)", "(Risk 8) [confidence 60.7%]") != base
