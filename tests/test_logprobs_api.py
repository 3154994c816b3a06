"""``logprobs`` / ``top_logprobs`` through the REST API (brain/api/protocol.py), the DP router and the lockstep TP
engine: reply shape for generate and chat, bytes that concatenate to the response, 400s, ``ignored_options`` on
backends that cannot, trimming at a stop string, the streamed final chunk."""
import asyncio
import json
import os

import pytest
import requests

from chronos.brain.api.server import FakeBackend
from test_api import Server, _port

CHAIN = ["[OPEN] attack_chain.sh -> /tmp/malware.bin", "[EXEC] attack_chain.sh -> curl"]


def _cfg(**kw):
    from chronos.brain.engine.engine import EngineConfig

    base = dict(model="tiny", device="cpu", max_slots=4, max_model_len=384, use_graphs=False, decode_burst=4)
    base.update(kw)
    return EngineConfig(**base)


@pytest.fixture(scope="module")
def service():
    from chronos.brain.api.service import EngineService

    svc = EngineService.from_config(_cfg(max_logprobs=5))
    s = Server(svc)
    yield s
    s.close()
    svc.close()


def _check_list(lps, text, top):
    assert isinstance(lps, list) and lps
    assert b"".join(bytes(e["bytes"]) for e in lps) == text.encode("utf-8")
    for e in lps:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
        assert isinstance(e["token"], str) and e["logprob"] <= 0.0 and len(e["top_logprobs"]) <= top
        for a in e["top_logprobs"]:
            assert set(a) == {"token", "logprob", "bytes"} and a["logprob"] <= 0.0
        lp = [a["logprob"] for a in e["top_logprobs"]]
        assert lp == sorted(lp, reverse=True)


def test_generate_and_chat_reply_shape(service):
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    body = requests.post(f"{service.url}/api/generate", timeout=120, json={
        "prompt": build_prompt(CHAIN), "format": VERDICT_SCHEMA, "stream": False, "logprobs": True, "top_logprobs": 3,
        "options": {"num_predict": 40}}).json()
    assert "ignored_options" not in body
    _check_list(body["logprobs"], body["response"], 3)
    assert len(body["logprobs"]) == body["eval_count"]
    assert any(e["logprob"] == 0.0 and len(e["top_logprobs"]) == 1 for e in body["logprobs"])  # grammar-forced tokens
    # greedy: the generated token is the first alternative
    assert all(e["top_logprobs"][0]["bytes"] == e["bytes"] for e in body["logprobs"])
    plain = requests.post(f"{service.url}/api/generate", timeout=120, json={
        "prompt": "hi", "stream": False, "logprobs": True, "options": {"num_predict": 6}}).json()
    _check_list(plain["logprobs"], plain["response"], 0)
    assert all(e["top_logprobs"] == [] for e in plain["logprobs"])
    many = requests.post(f"{service.url}/api/generate", timeout=120, json={
        "prompt": "hi", "stream": False, "logprobs": True, "top_logprobs": 20, "options": {"num_predict": 4}}).json()
    assert max(len(e["top_logprobs"]) for e in many["logprobs"]) == 5  # clamped to the engine's max_logprobs
    chat = requests.post(f"{service.url}/api/chat", timeout=120, json={
        "messages": [{"role": "user", "content": "hi"}], "stream": False, "logprobs": True, "top_logprobs": 2,
        "options": {"num_predict": 6}}).json()
    _check_list(chat["logprobs"], chat["message"]["content"], 2)
    off = requests.post(f"{service.url}/api/generate", timeout=120, json={
        "prompt": "hi", "stream": False, "options": {"num_predict": 4}}).json()
    assert "logprobs" not in off and "ignored_options" not in off
    assert off["response"] == many["response"]


@pytest.mark.parametrize("body", [{"logprobs": True, "top_logprobs": 21}, {"logprobs": True, "top_logprobs": -1},
                                  {"logprobs": True, "top_logprobs": "3"}, {"logprobs": True, "top_logprobs": True},
                                  {"logprobs": True, "top_logprobs": 2.5}, {"top_logprobs": 3},
                                  {"logprobs": False, "top_logprobs": 3}, {"logprobs": "yes"}, {"logprobs": 1}])
def test_bad_logprobs_fields_are_400(body):
    s = Server(FakeBackend("ok"))
    try:
        r = requests.post(f"{s.url}/api/generate", json=dict(body, prompt="x", stream=False), timeout=10)
        assert r.status_code == 400 and "logprobs" in r.json()["error"]
        r = requests.post(f"{s.url}/api/chat", timeout=10,
                          json=dict(body, messages=[{"role": "user", "content": "x"}], stream=False))
        assert r.status_code == 400
    finally:
        s.close()


def test_backends_that_cannot_report_ignored_option():
    from chronos.brain.api.service import EngineService

    s = Server(FakeBackend("ok"))
    try:
        b = requests.post(f"{s.url}/api/generate", json={"prompt": "x", "stream": False, "logprobs": True},
                          timeout=10).json()
        assert b["ignored_options"] == ["logprobs"] and "logprobs" not in b
        c = requests.post(f"{s.url}/api/chat", timeout=10, json={
            "messages": [{"role": "user", "content": "x"}], "stream": False, "logprobs": True}).json()
        assert c["ignored_options"] == ["logprobs"] and "logprobs" not in c
        r = requests.post(f"{s.url}/api/generate", json={"prompt": "x", "logprobs": True}, stream=True, timeout=10)
        last = [json.loads(l) for l in r.iter_lines() if l][-1]
        assert last["done"] and last["ignored_options"] == ["logprobs"]
    finally:
        s.close()
    svc = EngineService.from_config(_cfg(max_logprobs=0))
    s = Server(svc)
    try:
        b = requests.post(f"{s.url}/api/generate", timeout=120, json={
            "prompt": "x", "stream": False, "logprobs": True, "top_logprobs": 2, "options": {"num_predict": 4}}).json()
        assert b["ignored_options"] == ["logprobs"] and "logprobs" not in b and b["eval_count"] > 0
        assert svc.engine.stats["logprob_launches"] == 0 and svc.engine.s_lp is None
    finally:
        s.close()
        svc.close()


def test_stop_string_trims_the_list(service):
    req = {"prompt": "tell me", "stream": False, "logprobs": True, "top_logprobs": 1, "options": {"num_predict": 16}}
    full = requests.post(f"{service.url}/api/generate", json=req, timeout=120).json()
    text = full["response"]
    assert len(full["logprobs"]) >= 4
    # a stop string that begins inside a token where the text allows (that token is then not wholly inside the returned
    # text), else at a token boundary; it must first occur there, so the cut lands where the test expects
    tb = text.encode("utf-8")
    ends = [0]
    for e in full["logprobs"]:
        ends.append(ends[-1] + len(e["bytes"]))
    stop = None
    for inside in (1, 0):
        for k in range(1, len(full["logprobs"]) - 1):
            cut = ends[k] + (inside if ends[k + 1] - ends[k] > 1 else 0)
            try:
                head, cand = tb[:cut].decode("utf-8"), tb[cut:cut + 3].decode("utf-8")
            except UnicodeDecodeError:
                continue
            if cand and text.find(cand) == len(head):
                stop = cand
                break
        if stop:
            break
    assert stop, f"no usable stop string in {text!r}"
    cutb = requests.post(f"{service.url}/api/generate", timeout=120,
                         json=dict(req, options={"num_predict": 16, "stop": [stop]})).json()
    assert cutb["done_reason"] == "stop" and text.startswith(cutb["response"]) and cutb["response"] != text
    vis = cutb["response"].encode("utf-8")
    joined = b"".join(bytes(e["bytes"]) for e in cutb["logprobs"])
    assert vis.startswith(joined)
    n = len(cutb["logprobs"])
    assert cutb["logprobs"] == full["logprobs"][:n]
    assert n == len(full["logprobs"]) or not vis.startswith(joined + bytes(full["logprobs"][n]["bytes"]))


def test_streaming_last_chunk_carries_the_list(service):
    r = requests.post(f"{service.url}/api/generate", stream=True, timeout=120, json={
        "prompt": "hi", "format": "json", "logprobs": True, "top_logprobs": 2, "options": {"num_predict": 16}})
    lines = [json.loads(l) for l in r.iter_lines() if l]
    assert lines[-1]["done"] and all("logprobs" not in l for l in lines[:-1])
    _check_list(lines[-1]["logprobs"], "".join(l["response"] for l in lines), 2)


def test_dp_router_passes_logprobs_through():
    from chronos.brain.api.protocol import GenerateParams, logprobs_field
    from chronos.parallel.router import DPRouter
    from chronos.sensor.prompt import VERDICT_SCHEMA

    router = DPRouter(_cfg(max_logprobs=4), 1)
    try:
        async def go():
            ps = [GenerateParams(prompt="chain 0", stream=False, format=VERDICT_SCHEMA, num_predict=32, logprobs=2),
                  GenerateParams(prompt="chain 1", stream=False, format=VERDICT_SCHEMA, num_predict=32)]
            return await asyncio.gather(*[router.generate(p) for p in ps])

        a, b = asyncio.run(go())
        assert a.logprobs == 2 and len(a.out_logprobs) == len(a.out_ids) > 0
        assert b.logprobs == -1 and b.out_logprobs == []
        _check_list(logprobs_field(router.tok, a), a.text, 2)
        assert logprobs_field(router.tok, b) is None
    finally:
        router.close()


def _tp_worker(rank, world, port, q):
    import torch.distributed as dist

    from chronos.parallel.tp import TPContext
    from chronos.parallel.tp_engine import TPEngine
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = TPEngine(_cfg(max_logprobs=3), TPContext.from_group(), ctrl_group=None)
    seen, submit = [], eng.engine.submit

    def recording_submit(*a, **k):
        r = submit(*a, **k)
        seen.append(r)
        return r

    eng.engine.submit = recording_submit
    if rank == 0:
        eng.submit(build_prompt(CHAIN), fmt=VERDICT_SCHEMA, num_predict=30, logprobs=2)
        eng.submit(build_prompt(CHAIN[:1]), fmt=VERDICT_SCHEMA, num_predict=30)
        eng.run_until_idle()
    else:
        eng.follower_loop()
    q.put((rank, [(r.logprobs, list(r.out_ids), list(r.out_logprobs)) for r in seen]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.slow
def test_tp2_ranks_report_equal_lists():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    ps = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = dict(q.get(timeout=600) for _ in range(2))
    for p in ps:
        p.join(timeout=60)
    assert got[0] == got[1]  # every rank holds the all-gathered logits: equal ids and equal logprobs
    (want, ids, lps), (want2, ids2, lps2) = got[0]
    assert want == 2 and len(lps) == len(ids) > 0 and all(len(top) <= 2 for _, top in lps)
    assert want2 == -1 and lps2 == [] and ids2
