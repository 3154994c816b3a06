"""W4A16 decode GEMV (csrc/kernels/gemv.hip W4: OCP MXFP4 weights, bf16 activations): exact one-hot probes of every
position and every code, the dense ops against fp32 references of the same ops (plain, SwiGLU, the residual producer,
the folded-norm consumer, the QKV + RoPE + paged-KV epilogue on bf16 and fp8 caches) at the 8B decode shapes, the
mxfp4 model's decode step on the fp4 path against the same model on its bf16 copies, and the engine."""
import json

import pytest
import torch

from _mxfp4_cases import GRID, pack, probe_columns, spread_weight

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from chronos import ops

    ops.load()


@pytest.fixture
def max_m4():
    """The routing limit at the kernel's own (ops/gemm.py W4_MAX_M is 1 by default: only M = 1 measured faster than
    the bf16 kernels), so that the M = 2..4 instantiations are reached through chronos.ops and the model."""
    from chronos.ops import gemm

    old, gemm.W4_MAX_M = gemm.W4_MAX_M, 4
    try:
        yield
    finally:
        gemm.W4_MAX_M = old


def _q4(w):
    from chronos.models.llama import quantize_mxfp4

    return quantize_mxfp4(w.contiguous())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _probe(w4, cols, m, swiglu=False):
    """y[:, n] for one-hot rows of x at ``cols`` (m rows per launch) -> [len(cols), N] bf16."""
    n, k = w4.w.shape
    out = []
    for i in range(0, len(cols), m):
        js = cols[i:i + m]
        x = torch.zeros(len(js), k, device=DEV, dtype=torch.bfloat16)
        x[torch.arange(len(js)), torch.tensor(js)] = 1.0
        out.append(torch.ops.chronos.gemv(x, w4.q, swiglu, None, w4.e))
    return torch.cat(out)


def _want(w4, cols):
    # one exactly representable term plus zeros; a -0 term and +0 terms sum to +0 (IEEE), so -0 reads back as +0
    return (w4.w[:, torch.tensor(cols, device=DEV)].t().float() + 0.0).to(torch.bfloat16)


# ---- exact probes ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("m", [1, 2, 4])
@pytest.mark.parametrize("n", [16, 48])
@pytest.mark.parametrize("k", [1024, 2048, 3072, 5120])
def test_position_probe(k, n, m):
    """K = 1024: one chunk, three waves idle; 2048 / 3072: an even / odd chunk count; 5120: wave 0 takes two chunks."""
    w4 = _q4(spread_weight(n, k, 100 * m + n + k, DEV))
    assert w4.e.min().item() <= 114 and w4.e.max().item() >= 131  # the scales really differ from block to block
    cols = probe_columns(k, k + n)
    y = _probe(w4, cols, m)
    assert torch.equal(_bits(y), _bits(_want(w4, cols)))


def test_position_probe_persistent_groups():
    """knob gemv_persist = 2: two workgroups loop over the row groups with the next group's ring prefetched."""
    n, k, m = 48, 5120, 2
    w4 = _q4(spread_weight(n, k, 9, DEV))
    cols = probe_columns(k, 9)
    torch.ops.chronos.set_knob("gemv_persist", 2)
    try:
        y = _probe(w4, cols, m)
    finally:
        torch.ops.chronos.set_knob("gemv_persist", -1)
    assert torch.equal(_bits(y), _bits(_want(w4, cols)))


def test_code_table_probe():
    """Every code at the ends of the scale range.  Rows 0 / 1: all 16 codes in every block (in both nibbles) at
    e = 1 and e = 127.  Row 2: e = 254 with the 8 codes whose value is finite in bf16 (magnitudes 0 .. 1.5): 2, 3, 4
    and 6 times 2^127 overflow bf16, the reference table itself holds inf there, and a one-hot dot product over a row
    that contains inf is NaN by IEEE (0 * inf), so those 8 entries cannot be probed by any dot product.  Row 3: the
    three scales block by block."""
    from chronos.models.llama import Q4Tensor
    from chronos.ops import reference as ref

    n, k = 16, 1024
    all16 = torch.cat([torch.arange(16), torch.arange(15, -1, -1)])  # each code once per nibble position
    fin = torch.tensor([0, 1, 2, 3, 8, 9, 10, 11]).repeat(4)
    fin = torch.cat([fin[:16], fin[16:].flip(0)])
    codes = torch.zeros(n, k // 32, 32, dtype=torch.int32)
    e = torch.full((n, k // 32), 127, dtype=torch.uint8)
    codes[0], e[0] = all16, 1
    codes[1], e[1] = all16, 127
    codes[2], e[2] = fin, 254
    e[3] = torch.tensor([1, 127, 254]).repeat(11)[:k // 32].to(torch.uint8)
    codes[3] = torch.where((e[3] == 254)[:, None], fin[None, :], all16[None, :])
    q = pack(codes.reshape(n, k)).to(DEV)
    e = e.to(DEV)
    w4 = Q4Tensor(q, e, ref.dequantize_mxfp4(q, e))
    assert torch.isfinite(w4.w.float()).all()
    # the reference table in exact arithmetic
    mag = torch.tensor(GRID, dtype=torch.float64)[(codes & 7).long()]
    val = torch.where((codes & 8) != 0, -mag, mag) * torch.exp2(e.cpu().double() - 127)[..., None]
    assert torch.equal(w4.w.cpu().double(), val.reshape(n, k))
    cols = list(range(k))
    for m in (1, 2, 4):
        y = _probe(w4, cols, m)
        assert torch.equal(_bits(y), _bits(_want(w4, cols))), m


# ---- dense, against fp32 (the bound of test_w8a16_gpu.py) ----------------------------------------------------------


def _wx(m, n, k, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(m, k, device=DEV, generator=g) + 0.1).to(torch.bfloat16)
    w = (torch.randn(n, k, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    return x, _q4(w), g


def _close(y, want):
    err = (y.float() - want.float()).abs().max().item()
    print("max err", err, "max |want|", want.float().abs().max().item())
    assert err <= 1e-2 * want.float().abs().max().item() + 1e-3, (err, want.float().abs().max().item())


def _swiglu(full, n):
    gt, up = full[:, :n // 2].bfloat16().float(), full[:, n // 2:].bfloat16().float()
    return (gt / (1 + torch.exp(-gt))).bfloat16().float() * up


@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("n,k,swiglu", [(6144, 4096, False), (4096, 14336, False), (28672, 4096, True),
                                        (4096, 4096, False), (512, 1024, True)])
def test_gemv_w4a16(m, n, k, swiglu):
    x, w4, _ = _wx(m, n, k, m * n + k)
    y = torch.ops.chronos.gemv(x, w4.q, swiglu, None, w4.e)
    full = x.float() @ w4.w.float().t()
    want = _swiglu(full, n) if swiglu else full
    assert y.shape == want.shape
    _close(y, want)


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("n,k", [(4096, 4096), (4096, 14336)])
def test_gemv_resid_w4a16(m, n, k):
    x, w4, g = _wx(m, n, k, 7 * n + k + m)
    r = torch.randn(m, n, device=DEV, generator=g).to(torch.bfloat16)
    s = torch.empty_like(r)
    part = torch.ops.chronos.gemv_resid(x, w4.q, r, s, None, w4.e)
    want = ((x.float() @ w4.w.float().t()).bfloat16().float() + r.float())
    _close(s, want)
    torch.testing.assert_close(part.sum(1), (s.float() ** 2).sum(1), rtol=1e-3, atol=1e-2)


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("n,swiglu", [(6144, False), (28672, True)])
def test_gemv_normp_w4a16(m, n, swiglu):
    k = 4096
    x, w4, g = _wx(m, n, k, 11 * n + m)
    # producer: the fp4 residual GEMV writes s and its partial sums of squares
    wo = _q4((torch.randn(k, k, device=DEV, generator=g) * 0.02).to(torch.bfloat16))
    r = torch.randn(m, k, device=DEV, generator=g).to(torch.bfloat16)
    s = torch.empty_like(r)
    part = torch.ops.chronos.gemv_resid(x, wo.q, r, s, None, wo.e)
    y = torch.ops.chronos.gemv_normp(s, part, 1e-5, w4.q, swiglu, None, w4.e)
    sf = s.float()
    xn = sf * torch.rsqrt((sf * sf).mean(-1, keepdim=True) + 1e-5)
    full = xn @ w4.w.float().t()
    _close(y, _swiglu(full, n) if swiglu else full)


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("kv_fp8", [False, True])
def test_qkv_rope_w4a16_matches_unfused(m, kv_fp8, max_m4):
    from chronos import ops
    from chronos.models.llama import LlamaConfig, rope_table
    from chronos.ops import gemm

    hq, hkv, k = 32, 8, 4096
    n = (hq + 2 * hkv) * 128
    x, w4, g = _wx(m, n, k, 3 + m + 10 * kv_fp8)
    nb, bs = 64, 16
    dt = torch.uint8 if kv_fp8 else torch.bfloat16
    kc = torch.zeros(nb, hkv, bs, 128, device=DEV, dtype=dt)
    vc = torch.zeros(nb, hkv, 128, bs, device=DEV, dtype=dt)
    bt = torch.arange(1, 1 + 4 * m, device=DEV, dtype=torch.int32).view(m, 4)
    pos = torch.tensor([37, 50][:m], device=DEV, dtype=torch.int32)
    tok_seq = torch.arange(m, device=DEV, dtype=torch.int32)
    cs = rope_table(LlamaConfig(name="t"), 4096, DEV)
    ksc, vsc = (0.5, 0.25) if kv_fp8 else (1.0, 1.0)
    outs = []
    for fused in (True, False):
        k2, v2 = kc.clone(), vc.clone()
        q = torch.zeros(m, hq, 128, device=DEV, dtype=torch.bfloat16)
        if fused:
            before = gemm.w4_stats["gemv_launches"]
            assert ops.qkv_rope(x, w4, pos, tok_seq, bt, cs, q, k2, v2, hq, hkv, ksc, vsc)
            assert gemm.w4_stats["gemv_launches"] == before + 1  # the fp4 kernel, not the bf16 copy
        else:
            qkv = torch.ops.chronos.gemv(x, w4.q, False, None, w4.e)
            ops.rope_kv_write(qkv, pos, tok_seq, bt, cs, q, k2, v2, hq, hkv, True, ksc, vsc)
        outs.append((q, k2, v2))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    _close(torch.ops.chronos.gemv(x, w4.q, False, None, w4.e), x.float() @ w4.w.float().t())


def test_binding_checks():
    x, w4, _ = _wx(1, 32, 1024, 1)
    op = torch.ops.chronos.gemv
    with pytest.raises(RuntimeError):
        op(x, w4.q, False, None, w4.e[:, :16].contiguous())          # e is not [N, K / 32]
    with pytest.raises(RuntimeError):
        op(x, w4.w, False, None, w4.e)                               # w is not uint8
    with pytest.raises(RuntimeError):
        op(x[:, :512].contiguous(), w4.q[:, :256].contiguous(), False, None, w4.e[:, :16].contiguous())  # K % 1024
    with pytest.raises(RuntimeError):
        op(x.expand(5, -1).contiguous(), w4.q, False, None, w4.e)    # M <= 4
    with pytest.raises(RuntimeError):
        op(x, w4.q[:24].contiguous(), False, None, w4.e[:24].contiguous())  # N % 16
    with pytest.raises(RuntimeError):
        op(x, w4.q, False, torch.ones(32, device=DEV), w4.e)         # fp8 row scales and mxfp4 block scales together


# ---- model and engine --------------------------------------------------------------------------------------------


def test_default_routing_is_m1_only():
    """What is routed is what measured faster: M = 1.  M = 2..4 run the bf16 kernels on the copy."""
    from chronos import ops
    from chronos.ops import gemm

    assert gemm.W4_MAX_M == 1 and gemm._W4A16_DECODE
    x, w4, _ = _wx(4, 512, 1024, 2)
    c0 = gemm.w4_stats["gemv_launches"]
    y1 = ops.linear(x[:1], w4)
    assert gemm.w4_stats["gemv_launches"] == c0 + 1
    _close(y1, x[:1].float() @ w4.w.float().t())
    for m in (2, 3, 4):
        assert torch.equal(ops.linear(x[:m], w4), ops.linear(x[:m], w4.w))
        assert torch.equal(ops.gate_up_silu(x[:m], w4), ops.gate_up_silu(x[:m], w4.w))
    assert gemm.w4_stats["gemv_launches"] == c0 + 1


def test_mxfp4_model_decode_fp4_vs_bf16_copy(max_m4):
    from chronos.models.llama import KVCache, StepBatch, build_model, make_prefill_batch
    from chronos.ops import gemm

    m = build_model("small", DEV, seed=5, weight_dtype="mxfp4")
    assert m.w.w4 and not m.w.fp8
    prompt = list(range(100, 161))
    res, launches = {}, {}
    try:
        for name, on in (("fp4", True), ("copy", False)):
            gemm._W4A16_DECODE = on
            kv = KVCache(m.cfg, m.tp, 16, 16, DEV)
            bt = list(range(1, 6))
            sb = make_prefill_batch([prompt], [0], [bt], m.cfg, m.tp, DEV, max_blocks=8, nqt=8)
            m.forward(sb, kv)
            it = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
            bt_t = torch.zeros(1, 8, dtype=torch.int32, device=DEV)
            bt_t[0, :5] = it(bt)
            dec = StepBatch(it([777]), it([61]), it([0]), bt_t, it([0, 1]), it([62]),
                            torch.zeros(1, dtype=torch.int64, device=DEV), None, 1)
            c0 = gemm.w4_stats["gemv_launches"]
            res[name] = m.forward(dec, kv).float()
            c1 = gemm.w4_stats["gemv_launches"]
            jf = make_prefill_batch([[5, 6, 7]], [62], [bt], m.cfg, m.tp, DEV, max_blocks=8, nqt=2)
            res[name + "_jf"] = m.forward(jf, kv).float()
            launches[name] = (c1 - c0, gemm.w4_stats["gemv_launches"] - c1)
    finally:
        gemm._W4A16_DECODE = True
    L = m.cfg.num_layers
    # small: QKV, O and gate_up have K = 1024 (fp4); down has K = 2816, off the chunk, and runs on the bf16 copy
    # (the 3-row chunk: QKV and gate_up at least; O goes where the GEMM plan sends a 3-row residual producer)
    assert launches["fp4"][0] == 3 * L and launches["fp4"][1] >= 2 * L and launches["copy"] == (0, 0), launches
    cos = lambda a, b: torch.nn.functional.cosine_similarity(a, b, dim=-1).min().item()  # noqa: E731
    print("min cosine", cos(res["fp4"], res["copy"]), cos(res["fp4_jf"], res["copy_jf"]))
    assert cos(res["fp4"], res["copy"]) > 0.995
    assert cos(res["fp4_jf"], res["copy_jf"]) > 0.995


def test_mxfp4_engine_verdicts():
    from chronos.brain.engine.engine import Engine, EngineConfig
    from chronos.ops import gemm
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    chains = [["[OPEN] attack_chain.sh -> /tmp/malware.bin", "[EXEC] attack_chain.sh -> curl"],
              ["[EXEC] bash -> chmod", "[OPEN] chmod -> "],
              ["[EXEC] bash -> cat", "[OPEN] cat -> /tmp/malware.bin", "[EXEC] bash -> nc"],
              ["[EXEC] sshd -> bash", "[OPEN] bash -> /etc/shadow"]]
    eng = Engine(EngineConfig(model="small", device="cuda:0", max_slots=4, max_model_len=256, decode_burst=4,
                              weight_dtype="mxfp4"))
    assert eng.cfg.use_graphs and eng.model.w.w4
    before = gemm.w4_stats["gemv_launches"]
    # the first chain alone — the single-stream decode step, the one the default routing gives the fp4 kernel — then
    # the other three together
    reqs = [eng.submit(build_prompt(chains[0]), fmt=VERDICT_SCHEMA, num_predict=40)]
    eng.run_until_idle()
    alone = gemm.w4_stats["gemv_launches"] - before
    reqs += [eng.submit(build_prompt(c), fmt=VERDICT_SCHEMA, num_predict=40) for c in chains[1:]]
    eng.run_until_idle()
    torch.cuda.synchronize()
    assert alone >= 3 * eng.model.cfg.num_layers  # QKV, O and gate_up of every layer, at least one (captured) step
    for r in reqs:
        assert r.error is None
        assert {"risk_score", "verdict", "reason"} <= set(json.loads(r.text)), r.text
    assert gemm.w4_stats["gemv_launches"] >= before + alone
