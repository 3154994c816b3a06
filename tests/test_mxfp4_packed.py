"""Packed-only MXFP4 residency (weight_dtype "mxfp4-packed") on the CPU: the container without its bf16 copy, the
bit-equal model and engine, TP = 2 over gloo, the routing table of ops/gemm.py and the server surface."""
import asyncio
import json
import os
import socket

import pytest
import torch

CHAINS = [["[OPEN] attack_chain.sh -> /tmp/malware.bin", "[EXEC] attack_chain.sh -> curl"],
          ["[EXEC] bash -> chmod", "[OPEN] chmod -> "],
          ["[EXEC] bash -> cat", "[OPEN] cat -> /tmp/malware.bin", "[EXEC] bash -> nc"],
          ["[EXEC] sshd -> bash", "[OPEN] bash -> /etc/shadow"]]


@pytest.fixture(scope="module")
def tiny_pair():
    from chronos.models.llama import build_model

    return (build_model("tiny", "cpu", seed=3, weight_dtype="mxfp4"),
            build_model("tiny", "cpu", seed=3, weight_dtype="mxfp4-packed"))


def test_container_holds_only_the_packed_bytes(tiny_pair):
    from chronos import ops
    from chronos.models.llama import Q4Tensor

    mc, mp = tiny_pair
    assert mp.w.w4 is True and mp.w.fp8 is False
    assert mp.w.scratch is None and mp.w.scratch_nbytes() == 0  # a CPU model expands through the reference
    proj = 0
    for lc, lp in zip(mc.w.layers, mp.w.layers):
        for tc, tp_ in ((lc.wqkv, lp.wqkv), (lc.wo, lp.wo), (lc.w_gu, lp.w_gu), (lc.w_down, lp.w_down)):
            assert isinstance(tp_, Q4Tensor) and ops.is_w4(tp_) and not ops.is_q(tp_)
            assert tp_.w is None
            n, k = tp_.shape
            assert tuple(tp_.shape) == tuple(tc.shape) and tp_.numel() == tc.numel() == n * k
            assert tp_.nbytes() == n * k // 2 + n * k // 32
            assert torch.equal(tp_.q, tc.q) and torch.equal(tp_.e, tc.e)
            assert torch.equal(ops.w4_dense(tp_), tc.w) and ops.w4_dense(tc) is tc.w
            assert torch.equal(ops.w4_expand(tp_.q, tp_.e), tc.w)
            buf = torch.full((n * k + 64,), 7.0, dtype=torch.bfloat16)
            assert torch.equal(ops.w4_expand(tp_.q, tp_.e, buf), tc.w) and bool((buf[n * k:] == 7.0).all())
            proj += n * k
    assert mc.w.nbytes() - mp.w.nbytes() == 2 * proj  # exactly the copies


def test_quantize_keep_copy_flag():
    from chronos.models.llama import quantize_mxfp4

    w = torch.randn(8, 64).to(torch.bfloat16)
    a, b = quantize_mxfp4(w), quantize_mxfp4(w, keep_copy=False)
    assert a.w is not None and b.w is None and torch.equal(a.q, b.q) and torch.equal(a.e, b.e)
    assert tuple(b.shape) == (8, 64) and b.numel() == 512


def test_loaders_accept_the_mode():
    from chronos.models.llama import get_config, random_weights

    w = random_weights(get_config("tiny"), None, "cpu", 1, weight_dtype="mxfp4-packed")
    assert w.w4 and all(t.w is None for l in w.layers for t in (l.wqkv, l.wo, l.w_gu, l.w_down))


def test_prefill_and_decode_logits_equal_copy_mode(tiny_pair):
    from chronos.models.llama import KVCache, StepBatch, make_prefill_batch

    prompt = list(range(100, 131))
    outs = []
    for m in tiny_pair:
        kv = KVCache(m.cfg, m.tp, 8, 16, "cpu")
        bt = [1, 2, 3]
        pre = m.forward(make_prefill_batch([prompt], [0], [bt], m.cfg, m.tp, "cpu", max_blocks=4, nqt=8), kv)
        it = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
        bt_t = torch.zeros(1, 4, dtype=torch.int32)
        bt_t[0, :3] = it(bt)
        dec = StepBatch(it([777]), it([31]), it([0]), bt_t, it([0, 1]), it([32]), torch.zeros(1, dtype=torch.int64),
                        None, 1)
        outs.append((pre, m.forward(dec, kv)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _cfg(weights):
    from chronos.brain.engine.engine import EngineConfig

    return EngineConfig(model="tiny", device="cpu", max_slots=4, max_model_len=384, use_graphs=False, decode_burst=4,
                        weight_dtype=weights)


def _run_chains(weights):
    from chronos.brain.engine.engine import Engine
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    eng = Engine(_cfg(weights))
    assert eng.model.w.w4
    reqs = [eng.submit(build_prompt(c), fmt=VERDICT_SCHEMA, num_predict=40) for c in CHAINS]
    eng.run_until_idle()
    for r in reqs:
        assert r.error is None
    return eng, [(r.out_ids, r.text) for r in reqs]


@pytest.fixture(scope="module")
def copy_mode_chains():
    return _run_chains("mxfp4")[1]


def test_engine_texts_equal_copy_mode(copy_mode_chains):
    eng, got = _run_chains("mxfp4-packed")
    assert eng.model.w.layers[0].wqkv.w is None
    assert [t for _, t in got] == [t for _, t in copy_mode_chains]
    for _, t in got:
        assert {"risk_score", "verdict", "reason"} <= set(json.loads(t))


# ---- TP = 2 over gloo (the pattern of tests/test_tp_engine.py) ---------------------------------------------------------


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch.distributed as dist

    from chronos.parallel.tp import TPContext
    from chronos.parallel.tp_engine import TPEngine
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = TPEngine(_cfg("mxfp4-packed"), TPContext.from_group(), ctrl_group=None)
    assert eng.engine.model.w.w4 and eng.engine.model.w.layers[0].w_down.w is None
    if rank == 0:
        results = {}
        for i, c in enumerate(CHAINS[:2]):
            eng.submit(build_prompt(c), fmt=VERDICT_SCHEMA, num_predict=40,
                       callback=lambda r, i=i: results.__setitem__(i, (r.out_ids, r.text)))
        eng.run_until_idle()
        q.put(("leader", results))
    else:
        eng.follower_loop()
        q.put(("follower", dict(eng.engine.stats)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.slow
def test_tp2_packed_matches_copy_mode(copy_mode_chains):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = dict(q.get(timeout=600) for _ in range(2))
    for p in ps:
        p.join(timeout=60)
    res = got["leader"]
    assert sorted(res) == [0, 1] and got["follower"]["completed"] == 2
    for i in range(2):
        assert res[i][0] == copy_mode_chains[i][0], (i, res[i][1], copy_mode_chains[i][1])


# ---- routing table, pure Python -----------------------------------------------------------------------------------


def test_w4_plan_packed_takes_the_kernel_where_copy_mode_takes_the_copy():
    from chronos.ops import gemm

    assert gemm.W4_SKINNY == "plan" and gemm._W4A16_DECODE
    norow = (1024, 1024, gemm.PP_PLAIN)                       # never measured: no "w4plans" row
    lost = [(6144, 4096, gemm.PP_PLAIN), (28672, 4096, gemm.PP_SWIGLU)]  # rows whose M = 40-64 entries are -1
    w4plans = gemm._load_plans()["w4plans"]
    assert norow not in w4plans
    for n, k, mode in lost:
        assert w4plans[(n, k, mode)][-1][:2] == [64, -1]
    for m in (2, 40, 48, 64):
        assert gemm.w4_plan(m, *norow) is None
        got = gemm.w4_plan(m, *norow, packed=True)
        assert got is not None and got == gemm._sk4_model(m, *norow) and gemm._sk4_valid(got[0], m, *norow, got[1])
    for n, k, mode in lost:
        for m in (40, 48, 64):
            assert gemm.w4_plan(m, n, k, mode) is None
            got = gemm.w4_plan(m, n, k, mode, packed=True)
            assert got is not None and got == gemm._sk4_model(m, n, k, mode)
        # a winning row is the same in both modes
        assert gemm.w4_plan(8, n, k, mode, packed=True) == gemm.w4_plan(8, n, k, mode) is not None
    assert gemm.w4_plan(65, *norow, packed=True) is None  # above the kernel's M: the expansion
    assert gemm.w4_plan(16, 1024, 2816, gemm.PP_PLAIN, packed=True) is None  # K the kernel does not take


def test_w4_plan_packed_keeps_the_switches(monkeypatch):
    from chronos.ops import gemm

    monkeypatch.setattr(gemm, "W4_SKINNY", "off")
    assert gemm.w4_plan(16, 1024, 1024, gemm.PP_PLAIN, packed=True) is None
    monkeypatch.setattr(gemm, "W4_SKINNY", "plan")
    monkeypatch.setattr(gemm, "_W4A16_DECODE", False)
    assert gemm.w4_plan(16, 1024, 1024, gemm.PP_PLAIN, packed=True) is None
    assert "expand_launches" in gemm.w4_stats


# ---- server ---------------------------------------------------------------------------------------------------------


def test_server_cli_and_scripts_accept_the_mode():
    from chronos.brain.api.server import build_parser

    assert build_parser().parse_args(["--weights", "mxfp4-packed"]).weights == "mxfp4-packed"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for script in ("single_stream.py", "fw_bucket.py", "long_context.py"):
        src = open(os.path.join(root, "scripts", script)).read()
        assert '"mxfp4-packed"' in next(l for l in src.splitlines() if '"--weights"' in l)
    bench = open(os.path.join(root, "bench.py")).read()
    assert "mxfp4-packed" not in bench


def test_endpoints_report_mxfp4_and_resident_bytes():
    from aiohttp.test_utils import TestClient, TestServer

    from chronos.brain.api.server import make_app
    from chronos.brain.api.service import EngineService
    from chronos.brain.engine.engine import EngineConfig

    svc = EngineService.from_config(EngineConfig(model="tiny", device="cpu", max_slots=2, max_model_len=128,
                                                 use_graphs=False, weight_dtype="mxfp4-packed"))

    async def go():
        async with TestClient(TestServer(make_app(svc))) as c:
            tags = await (await c.get("/api/tags")).json()
            ps = await (await c.get("/api/ps")).json()
            show = await (await c.post("/api/show", json={"model": "llama3"})).json()
            return tags, ps, show

    try:
        tags, ps, show = asyncio.run(go())
        w = svc.engine.model.w
        assert tags["models"][0]["details"]["quantization_level"] == "MXFP4"
        assert ps["models"][0]["details"]["quantization_level"] == "MXFP4"
        assert show["details"]["quantization_level"] == "MXFP4"
        assert ps["models"][0]["size_vram"] == w.nbytes() + w.scratch_nbytes() < ps["models"][0]["size"]
    finally:
        svc.close()
