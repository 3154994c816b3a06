"""MXFP4 projection weights on the CPU: the OCP MX v1.0 quantiser (hand-worked blocks, fixed point, exactness, error
of a Gaussian tensor), the Q4Tensor container and its loading, the model forward against a bf16 model holding the
dequantised copies, TP = 2 over gloo, the server CLI / endpoints and the routing predicate."""
import asyncio
import json
import os
import socket

import pytest
import torch

from _mxfp4_cases import GRID, TIES, block, codes_of, pack, table_value


def _ref():
    from chronos.ops import reference

    return reference


# ---- quantiser ------------------------------------------------------------------------------------------------------


def test_ties_to_even_code_both_signs():
    ref = _ref()
    vals = [v for v, _ in TIES]
    q, e = ref.quantize_mxfp4(block(vals))
    assert e.tolist() == [[127]]  # amax 5: floor(log2) = 2, X = 0
    assert codes_of(q)[0, :len(vals)].tolist() == [c for _, c in TIES]
    deq = ref.dequantize_mxfp4(q, e).float()[0, :len(vals)].tolist()
    assert deq == [table_value(c, 127) for _, c in TIES]


def test_saturation_to_six():
    ref = _ref()
    q, e = ref.quantize_mxfp4(block([7.9, -7.9, 1.0]))  # amax 7.9: X = 0, 7.9 lies above the grid
    assert e.tolist() == [[127]]
    assert codes_of(q)[0, :3].tolist() == [7, 15, 2]
    assert ref.dequantize_mxfp4(q, e).float()[0, :3].tolist() == [6.0, -6.0, 1.0]


def test_all_zero_block():
    ref = _ref()
    q, e = ref.quantize_mxfp4(torch.zeros(2, 64, dtype=torch.bfloat16))
    assert e.tolist() == [[127, 127]] * 2 and int(q.sum()) == 0
    assert torch.equal(ref.dequantize_mxfp4(q, e), torch.zeros(2, 64, dtype=torch.bfloat16))


def test_exponent_clamp():
    ref = _ref()
    # amax 2^-125: X = -127 would be e = 0, which is no f32 normal; e clamps to 1 (scale 2^-126) and the element is
    # 2^-125 / 2^-126 = 2 instead of 4
    q, e = ref.quantize_mxfp4(block([2.0 ** -125, -(2.0 ** -126)]))
    assert e.tolist() == [[1]]
    assert codes_of(q)[0, :2].tolist() == [4, 10]
    assert ref.dequantize_mxfp4(q, e).float()[0, :2].tolist() == [2.0 ** -125, -(2.0 ** -126)]
    # a bf16 subnormal block far below the clamp rounds to zero
    q, e = ref.quantize_mxfp4(block([2.0 ** -130]))
    assert e.tolist() == [[1]] and codes_of(q)[0, 0].item() == 0
    # the largest finite bf16 needs no clamp: floor(log2) = 127 -> e = 252
    q, e = ref.quantize_mxfp4(block([3.0 * 2.0 ** 126]))
    assert e.tolist() == [[252]] and codes_of(q)[0, 0].item() == 7


def test_nibble_and_byte_order():
    ref = _ref()
    w = torch.zeros(1, 64)
    w[0, :3] = torch.tensor([6.0, -4.0, 0.5])
    w[0, 32:35] = torch.tensor([0.0, 3.0, -3.0])  # second block: amax 3 -> X = -1, e = 126: 3 -> 6
    q, e = ref.quantize_mxfp4(w.to(torch.bfloat16))
    assert q.shape == (1, 32) and e.shape == (1, 2) and q.dtype == torch.uint8 and e.dtype == torch.uint8
    assert e.tolist() == [[127, 126]]
    assert q[0, :2].tolist() == [0x7 | (0xE << 4), 0x1]  # element 0 low nibble, element 1 high nibble
    assert q[0, 16:18].tolist() == [0x7 << 4, 0xF]
    assert int(q[0, 2:16].sum()) == 0 and int(q[0, 18:].sum()) == 0


def test_fixed_point():
    ref = _ref()
    g = torch.Generator().manual_seed(0)
    q = torch.randint(0, 256, (64, 512), generator=g).to(torch.uint8)
    e = torch.randint(100, 141, (64, 32), generator=g).to(torch.uint8)
    w = ref.dequantize_mxfp4(q, e)
    q2, e2 = ref.quantize_mxfp4(w)
    w2 = ref.dequantize_mxfp4(q2, e2)
    assert torch.equal(w.view(torch.int16), w2.view(torch.int16))


def test_dequantised_values_are_exact_in_bf16():
    ref = _ref()
    g = torch.Generator().manual_seed(1)
    q = torch.randint(0, 256, (32, 256), generator=g).to(torch.uint8)
    e = torch.randint(1, 253, (32, 16), generator=g).to(torch.uint8)  # 6 * 2^(e - 127) stays finite in bf16
    w = ref.dequantize_mxfp4(q, e)
    c = codes_of(q)
    mag = torch.tensor(GRID)[(c & 7).long()]
    val = torch.where((c & 8) != 0, -mag, mag).double()
    want = val * torch.exp2(e.double() - 127).repeat_interleave(32, dim=1)
    assert torch.equal(w.double(), want)


@pytest.mark.parametrize("sigma", [0.02, 1.0])
def test_gaussian_error(sigma):
    ref = _ref()
    g = torch.Generator().manual_seed(2)
    w = (torch.randn(512, 4096, generator=g) * sigma).to(torch.bfloat16)
    q, e = ref.quantize_mxfp4(w)
    d = ref.dequantize_mxfp4(q, e).float() - w.float()
    rel = (d.norm() / w.float().norm()).item()
    print("relative Frobenius error", sigma, rel)
    assert rel < 0.13


# ---- container, loading, model -----------------------------------------------------------------------------------


def test_unknown_weight_dtype_names_the_valid_ones():
    from chronos.models.llama import build_model

    with pytest.raises(ValueError) as ei:
        build_model("tiny", "cpu", weight_dtype="int4")
    for name in ("bf16", "fp8", "mxfp4"):
        assert name in str(ei.value)


@pytest.fixture(scope="module")
def tiny_models():
    from chronos.models.llama import build_model

    m4 = build_model("tiny", "cpu", seed=3, weight_dtype="mxfp4")
    mb = build_model("tiny", "cpu", seed=3)
    for l4, lb in zip(m4.w.layers, mb.w.layers):  # the bf16 model runs on the dequantised copies
        lb.wqkv, lb.wo, lb.w_gu, lb.w_down = l4.wqkv.w, l4.wo.w, l4.w_gu.w, l4.w_down.w
    return m4, mb


def test_container_and_flags(tiny_models):
    from chronos import ops
    from chronos.models.llama import Q4Tensor

    m4, mb = tiny_models
    w = m4.w
    assert w.w4 is True and w.fp8 is False and mb.w.w4 is False
    lw = w.layers[0]
    ref = _ref()
    for t in (lw.wqkv, lw.wo, lw.w_gu, lw.w_down):
        assert isinstance(t, Q4Tensor) and ops.is_w4(t) and not ops.is_q(t)
        n, k = t.shape
        assert t.q.shape == (n, k // 2) and t.e.shape == (n, k // 32) and t.w.shape == (n, k)
        assert t.w.dtype == torch.bfloat16 and t.w.is_contiguous() and t.numel() == n * k
        assert t.nbytes() == n * k // 2 + n * k // 32 + 2 * n * k
        assert torch.equal(t.w, ref.dequantize_mxfp4(t.q, t.e))
    assert isinstance(w.embed, torch.Tensor) and isinstance(w.lm_head, torch.Tensor)
    assert isinstance(lw.attn_norm, torch.Tensor)
    proj = sum(t.numel() for l in w.layers for t in (l.wqkv, l.wo, l.w_gu, l.w_down))
    assert w.nbytes() - mb.w.nbytes() == proj // 2 + proj // 32  # q and e on top of the bf16 bytes


def test_model_forward_equals_bf16_on_the_copies(tiny_models):
    from chronos.models.llama import KVCache, StepBatch, make_prefill_batch

    m4, mb = tiny_models
    prompt = list(range(100, 131))
    outs = []
    for m in (m4, mb):
        kv = KVCache(m.cfg, m.tp, 8, 16, "cpu")
        bt = [1, 2, 3]
        sb = make_prefill_batch([prompt], [0], [bt], m.cfg, m.tp, "cpu", max_blocks=4, nqt=8)
        pre = m.forward(sb, kv)
        it = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
        bt_t = torch.zeros(1, 4, dtype=torch.int32)
        bt_t[0, :3] = it(bt)
        dec = StepBatch(it([777]), it([31]), it([0]), bt_t, it([0, 1]), it([32]), torch.zeros(1, dtype=torch.int64),
                        None, 1)
        outs.append((pre, m.forward(dec, kv)))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


def test_shards_quantise_like_the_whole():
    """Quantisation happens after TP sharding.  A row-parallel shard's K-slice starts on an MX block boundary
    whenever K / world is a multiple of 32, so its blocks are the unsharded tensor's blocks."""
    from chronos.models.llama import get_config, random_weights
    from chronos.parallel.tp import TPContext

    cfg = get_config("tiny")
    full = random_weights(cfg, None, "cpu", 4, weight_dtype="mxfp4").layers[0]
    hq, hkv, D = cfg.num_heads // 2, cfg.num_kv_heads // 2, cfg.head_dim
    for r in range(2):
        sh = random_weights(cfg, TPContext(rank=r, world=2), "cpu", 4, weight_dtype="mxfp4").layers[0]
        kq = full.wo.shape[1] // 2
        assert torch.equal(sh.wo.w, full.wo.w[:, r * kq:(r + 1) * kq])
        kd = full.w_down.shape[1] // 2
        assert torch.equal(sh.w_down.w, full.w_down.w[:, r * kd:(r + 1) * kd])
        assert torch.equal(sh.wqkv.w[:hq * D], full.wqkv.w[r * hq * D:(r + 1) * hq * D])


# ---- TP = 2 over gloo ------------------------------------------------------------------------------------------------

CHAINS = [["[OPEN] attack_chain.sh -> /tmp/malware.bin", "[EXEC] attack_chain.sh -> curl"],
          ["[EXEC] bash -> chmod", "[OPEN] chmod -> "]]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cfg():
    from chronos.brain.engine.engine import EngineConfig

    return EngineConfig(model="tiny", device="cpu", max_slots=4, max_model_len=384, use_graphs=False, decode_burst=4,
                        weight_dtype="mxfp4")


def _worker(rank, world, port, q):
    import torch.distributed as dist

    from chronos.parallel.tp import TPContext
    from chronos.parallel.tp_engine import TPEngine
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = TPEngine(_cfg(), TPContext.from_group(), ctrl_group=None)
    assert eng.engine.model.w.w4
    if rank == 0:
        results = {}
        for i, c in enumerate(CHAINS):
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
def test_tp2_mxfp4_matches_tp1():
    import torch.multiprocessing as mp

    from chronos.brain.engine.engine import Engine
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    ref = Engine(_cfg())
    assert ref.model.w.w4
    reqs = [ref.submit(build_prompt(c), fmt=VERDICT_SCHEMA, num_predict=40) for c in CHAINS]
    ref.run_until_idle()
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
    for i, r in enumerate(reqs):
        assert res[i][0] == r.out_ids, (i, res[i][1], r.text)
        assert set(json.loads(res[i][1])) == {"risk_score", "verdict", "reason"}


# ---- CLI, endpoints, routing predicate -----------------------------------------------------------------------------


def test_server_cli_parses_weights():
    from chronos.brain.api.server import build_parser

    ap = build_parser()
    assert ap.parse_args([]).weights == "bf16"
    assert ap.parse_args(["--weights", "mxfp4"]).weights == "mxfp4"
    assert ap.parse_args(["--weights", "fp8", "--kv-dtype", "fp8"]).weights == "fp8"
    with pytest.raises(SystemExit):
        ap.parse_args(["--weights", "int4"])


@pytest.mark.parametrize("script", ["single_stream.py", "fw_bucket.py", "long_context.py"])
def test_scripts_accept_mxfp4(script):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", script)).read()
    line = next(l for l in src.splitlines() if '"--weights"' in l)
    assert '"mxfp4"' in line


def _levels(backend):
    from aiohttp.test_utils import TestClient, TestServer

    from chronos.brain.api.server import make_app

    async def go():
        async with TestClient(TestServer(make_app(backend))) as c:
            tags = await (await c.get("/api/tags")).json()
            ps = await (await c.get("/api/ps")).json()
            show = await (await c.post("/api/show", json={"model": "llama3"})).json()
            return (tags["models"][0]["details"]["quantization_level"],
                    ps["models"][0]["details"]["quantization_level"], show["details"]["quantization_level"])

    return asyncio.run(go())


@pytest.mark.parametrize("weights,level", [("mxfp4", "MXFP4"), ("bf16", "BF16")])
def test_endpoints_report_quantization_level(weights, level):
    from chronos.brain.api.service import EngineService
    from chronos.brain.engine.engine import EngineConfig

    kw = {} if weights == "bf16" else {"weight_dtype": weights}
    svc = EngineService.from_config(EngineConfig(model="tiny", device="cpu", max_slots=2, max_model_len=128,
                                                 use_graphs=False, **kw))
    try:
        assert _levels(svc) == (level,) * 3
    finally:
        svc.close()


def test_fake_backend_still_says_bf16():
    from chronos.brain.api.server import FakeBackend

    assert _levels(FakeBackend("ok")) == ("BF16",) * 3


def test_routing_predicate():
    from chronos import ops

    for m in (1, 2, 3, 4):
        for n, k in ((6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)):
            assert ops.gemv_w4_ok(m, n, k)
        assert not ops.gemv_w4_ok(m, 8192, 3584)  # the 70B TP = 8 down-projection shard
        assert ops.gemv_w4_ok(m, 8192, 1024)      # ... and its O-projection shard
    assert not ops.gemv_w4_ok(5, 4096, 4096) and not ops.gemv_w4_ok(1, 4104, 4096)


def test_cpu_ops_run_on_the_copy():
    """On the CPU every op takes ``.w``: the result is the bf16 op's, bit for bit, and nothing is counted."""
    from chronos import ops
    from chronos.models.llama import quantize_mxfp4
    from chronos.ops import gemm

    g = torch.Generator().manual_seed(5)
    w = quantize_mxfp4((torch.randn(64, 1024, generator=g) * 0.05).to(torch.bfloat16))
    x = torch.randn(2, 1024, generator=g).to(torch.bfloat16)
    before = gemm.w4_stats["gemv_launches"]
    assert torch.equal(ops.linear(x, w), ops.linear(x, w.w))
    assert torch.equal(ops.gate_up_silu(x, w), ops.gate_up_silu(x, w.w))
    assert gemm.w4_stats["gemv_launches"] == before
