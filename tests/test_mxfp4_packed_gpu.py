"""Packed-only MXFP4 residency on the GPU: the expansion kernel (csrc/kernels/w4_expand.hip) bit for bit against
ops.reference.dequantize_mxfp4 — every (byte, scale) pair, tails, a wrapping grid, sentinels, the decode gate, the
binding's checks — and the packed-only model and engine against copy mode by bit equality."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 4096  # sentinel elements on each side of ``out``
SENT = 0x7E57  # a bf16 bit pattern no expansion of the inputs below produces next to the buffer


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from chronos import ops

    ops.load()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ref(q, e):
    """The reference on the CPU (its f32 product keeps the one subnormal of the table)."""
    from chronos.ops import reference

    return reference.dequantize_mxfp4(q.cpu(), e.cpu())


def _padded(n, k):
    buf = torch.full((n * k + 2 * PAD,), SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return buf, buf[PAD:PAD + n * k]


def _sentinels_intact(buf, n, k):
    b = _bits(buf)
    return bool((b[:PAD] == SENT).all()) and bool((b[PAD + n * k:] == SENT).all())


# ---- the kernel -----------------------------------------------------------------------------------------------------


def test_every_byte_and_scale_pair():
    """q [254, 256]: every byte value once per row (so every code in both nibbles); e[r, :] = r + 1: every scale 1-254.
    Bit equality with the reference for every pair but one: magnitude code 1 (0.5) at e = 1, whose value 2^-127 is a
    bf16 subnormal (0x0040 / 0x8040) — there a signed zero of the same sign is accepted too.  The MI355X keeps the
    subnormal in all 64 places (the test prints the count)."""
    from chronos import ops

    g = torch.Generator().manual_seed(11)
    q = torch.stack([torch.randperm(256, generator=g) for _ in range(254)]).to(torch.uint8).to(DEV)
    e = (torch.arange(254, dtype=torch.int32) + 1).to(torch.uint8).view(254, 1).repeat(1, 16).contiguous().to(DEV)
    got = _bits(ops.w4_expand(q, e)).cpu()
    ref = _bits(_ref(q, e))
    assert got.shape == ref.shape == (254, 512)
    qi = q.cpu().to(torch.int32)
    code = torch.stack([qi & 15, qi >> 4], -1).reshape(254, 512)
    sub = ((code & 7) == 1) & (torch.arange(254).view(-1, 1) == 0)  # 0.5 * 2^-126
    assert int(sub.sum()) == 2 * 2 * 16  # both signs, both nibbles, 16 bytes each
    assert bool((ref[sub] & 0x7FFF == 0x0040).all())
    assert torch.equal(got[~sub], ref[~sub])
    zero = ref[sub] & ~0x7FFF  # the same sign, magnitude 0
    kept = int((got[sub] == ref[sub]).sum())
    print(f"code 1 at e = 1: the hardware kept the subnormal in {kept} of {int(sub.sum())} places, "
          f"returned a signed zero in {int((got[sub] == zero).sum())}")
    assert bool(((got[sub] == ref[sub]) | (got[sub] == zero)).all())


@pytest.mark.parametrize("n,k", [(1, 32), (3, 96), (17, 1056), (512, 1024), (4096, 4096)])
def test_shapes_tails_and_sentinels(n, k):
    """One piece, a partial wave, K / 8 no multiple of 64, several tiles, and (4096, 4096): 2048 tiles over the grid of
    at most 1024 workgroups, so the grid-stride loop wraps.  ``out`` is a slice of a larger buffer."""
    from chronos import ops

    g = torch.Generator().manual_seed(n * 7 + k)
    q = torch.randint(0, 256, (n, k // 2), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    e = torch.randint(2, 255, (n, k // 32), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    buf, out = _padded(n, k)
    y = ops.w4_expand(q, e, out)
    torch.cuda.synchronize()
    assert y.shape == (n, k) and y.data_ptr() == out.data_ptr()
    assert torch.equal(_bits(y).cpu(), _bits(_ref(q, e)))
    assert _sentinels_intact(buf, n, k)


def test_out_may_be_longer_than_the_matrix():
    from chronos import ops

    n, k = 5, 64
    g = torch.Generator().manual_seed(3)
    q = torch.randint(0, 256, (n, k // 2), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    e = torch.full((n, k // 32), 127, dtype=torch.uint8, device=DEV)
    buf, _ = _padded(n, k)
    y = ops.w4_expand(q, e, buf[PAD:])  # n k + PAD elements: only the first n k are written
    assert torch.equal(_bits(y).cpu(), _bits(_ref(q, e))) and _sentinels_intact(buf, n, k)


def test_decode_gate():
    from chronos import ops

    n, k = 64, 1024
    g = torch.Generator().manual_seed(5)
    q = torch.randint(0, 256, (n, k // 2), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    e = torch.full((n, k // 32), 120, dtype=torch.uint8, device=DEV)
    buf, out = _padded(n, k)
    state = torch.zeros(8, dtype=torch.int32, device=DEV)  # DONE everywhere: no live row
    state[5] = 3  # live, but outside the gate's n = 4 rows
    try:
        ops.set_decode_gate(state, 4)
        ops.w4_expand(q, e, out)
        torch.cuda.synchronize()
        assert bool((_bits(buf) == SENT).all())
        state[2] = 5  # one live row: the same launch writes
        ops.w4_expand(q, e, out)
        torch.cuda.synchronize()
    finally:
        ops.set_decode_gate(None, 0)
    assert torch.equal(_bits(out).view(n, k).cpu(), _bits(_ref(q, e))) and _sentinels_intact(buf, n, k)


def test_binding_checks():
    n, k = 4, 64
    q = torch.zeros(n, k // 2, dtype=torch.uint8, device=DEV)
    e = torch.full((n, k // 32), 127, dtype=torch.uint8, device=DEV)
    out = torch.zeros(n * k + 8, dtype=torch.bfloat16, device=DEV)
    f = torch.ops.chronos.w4_expand
    f(q, e, out)  # the good call
    with pytest.raises(RuntimeError, match="uint8"):
        f(q.to(torch.int8), e, out)
    with pytest.raises(RuntimeError, match="uint8"):
        f(q, e.to(torch.int32), out)
    with pytest.raises(RuntimeError, match="bfloat16"):
        f(q, e, out.to(torch.float16))
    with pytest.raises(RuntimeError, match=r"K / 32"):
        f(q, torch.full((n, k // 32 + 1), 127, dtype=torch.uint8, device=DEV), out)
    with pytest.raises(RuntimeError, match=r"K / 32"):
        f(q, e[:n - 1].contiguous(), out)
    with pytest.raises(RuntimeError, match="K % 32"):
        f(q[:, :24].contiguous(), e[:, :1].contiguous(), out)
    with pytest.raises(RuntimeError, match="fewer than N K"):
        f(q, e, out[:n * k - 8])
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        f(q, e, out[1:])
    with pytest.raises(RuntimeError, match="contiguous"):
        f(q.t().contiguous().t(), e, out)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        f(q, e.cpu(), out)
    torch.cuda.synchronize()


# ---- model ------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def small_pair():
    from chronos.models.llama import build_model

    return (build_model("small", DEV, seed=5, weight_dtype="mxfp4"),
            build_model("small", DEV, seed=5, weight_dtype="mxfp4-packed"))


@pytest.fixture
def dense_route():
    """CHRONOS_W4A16_DECODE=0 for one test: no W4A16 kernel, so packed-only expands everywhere."""
    from chronos.ops import gemm

    old = gemm._W4A16_DECODE
    gemm._W4A16_DECODE = False
    try:
        yield
    finally:
        gemm._W4A16_DECODE = old


def _it(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _prefill_and_decode4(m):
    """A 4 x 61-token prefill (M = 244) and the 4-row decode step after it: (logits, logits, launches of each)."""
    from chronos.models.llama import KVCache, StepBatch, make_prefill_batch
    from chronos.ops import gemm

    prompts = [list(range(100 + 7 * b, 161 + 7 * b)) for b in range(4)]
    bts = [list(range(1 + 5 * b, 6 + 5 * b)) for b in range(4)]
    kv = KVCache(m.cfg, m.tp, 32, 16, DEV)
    kv.buf.zero_()
    c0 = dict(gemm.w4_stats)
    pre = m.forward(make_prefill_batch(prompts, [0] * 4, bts, m.cfg, m.tp, DEV, max_blocks=8, nqt=8), kv)
    c1 = dict(gemm.w4_stats)
    bt_t = torch.zeros(4, 8, dtype=torch.int32, device=DEV)
    for b in range(4):
        bt_t[b, :5] = _it(bts[b])
    dec = StepBatch(_it([777, 778, 779, 780]), _it([61] * 4), _it([0, 1, 2, 3]), bt_t, _it([0, 1, 2, 3, 4]),
                    _it([62] * 4), torch.arange(4, dtype=torch.int64, device=DEV), None, 4)
    out = m.forward(dec, kv)
    c2 = dict(gemm.w4_stats)
    d = lambda a, b: {k: b[k] - a[k] for k in b}  # noqa: E731
    return pre, out, d(c0, c1), d(c1, c2)


def _decode80(m):
    """An 80-row decode step (above the W4A16 kernels' M) over a seeded KV cache."""
    from chronos import ops
    from chronos.models.llama import KVCache, StepBatch
    from chronos.ops import gemm

    n, bs, ctx_max = 80, 16, 20
    nbs = (ctx_max + 1 + bs - 1) // bs
    kv = KVCache(m.cfg, m.tp, n * nbs + 1, bs, DEV)
    kv.buf.normal_(0, 0.5, generator=torch.Generator(device=DEV).manual_seed(9))
    bt = (torch.arange(n * nbs, dtype=torch.int32, device=DEV) + 1).view(n, nbs)
    ctx = _it([ctx_max - (i % 7) for i in range(n)])
    ar = torch.arange(n + 1, dtype=torch.int32, device=DEV)
    ids = (torch.arange(n, dtype=torch.int32, device=DEV) * 37 + 11) % m.cfg.vocab_size
    sb = StepBatch(ids, ctx - 1, ar[:n], bt, ar, ctx, torch.arange(n, dtype=torch.int64, device=DEV), None, n, 1,
                   ops.pick_nsplit(n * m.hkv, ctx_max + 1))
    c0 = gemm.w4_stats["expand_launches"]
    out = m.forward(sb, kv)
    return out, gemm.w4_stats["expand_launches"] - c0


def test_packed_model_holds_no_copy_and_one_scratch(small_pair):
    mc, mp = small_pair
    assert mp.w.w4 and mc.w.scratch is None
    q4 = [t for l in mp.w.layers for t in (l.wqkv, l.wo, l.w_gu, l.w_down)]
    assert all(t.w is None and t.scratch is mp.w.scratch for t in q4)
    assert mp.w.scratch.buf.numel() == max(t.numel() for t in q4) and mp.w.scratch.buf.data_ptr() % 16 == 0
    assert mp.w.nbytes() + mp.w.scratch_nbytes() < mc.w.nbytes()


def test_scratch_reuse_across_streams(small_pair, dense_route):
    """Two projections expanded into the one scratch from two different streams, each followed by its GEMM on that
    stream: the second stream waits for the first one's work (W4Scratch.acquire), so both products are copy mode's."""
    from chronos import ops

    mc, mp = small_pair
    lc, lp = mc.w.layers[0], mp.w.layers[0]
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(200, lc.wqkv.shape[1], device=DEV, generator=g).to(torch.bfloat16)
    want = (ops.linear(x, lc.wqkv), ops.linear(x, lc.wo))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = ops.linear(x, lp.wqkv)
    assert mp.w.scratch._stream == s1
    with torch.cuda.stream(s2):
        b = ops.linear(x, lp.wo)
    assert mp.w.scratch._stream == s2
    torch.cuda.synchronize()
    assert torch.equal(a, want[0]) and torch.equal(b, want[1])


def test_packed_model_equals_copy_mode_on_the_dense_route(small_pair, dense_route):
    mc, mp = small_pair
    L = mc.cfg.num_layers
    pc, dc, _, _ = _prefill_and_decode4(mc)
    pp, dp, n_pre, n_dec = _prefill_and_decode4(mp)
    assert torch.equal(pc, pp) and torch.equal(dc, dp)
    assert n_pre["expand_launches"] == 4 * L and n_dec["expand_launches"] == 4 * L
    assert n_pre["skinny_launches"] == n_dec["skinny_launches"] == n_dec["gemv_launches"] == 0
    bc, nc = _decode80(mc)
    bp, np_ = _decode80(mp)
    assert torch.equal(bc, bp) and nc == 0 and np_ == 4 * L


def test_default_routing_small_batch_takes_the_w4_kernels(small_pair):
    """Default routing, 4-row decode: every projection the W4A16 skinny kernel accepts runs on it and issues no
    expansion.  On "small" that is QKV, O and gate_up (K = 1024); down has K = 2816 = 22 x 128, which no skinny
    config's wave count divides (tests/test_mxfp4_skinny_gpu.py), so it alone expands, once per layer.  With the MLP
    width at 3072 (24 x 128) all four projections are accepted and the step issues no expansion at all."""
    from dataclasses import replace

    from chronos.models.llama import build_model, get_config
    from chronos.ops import gemm

    assert gemm._W4A16_DECODE and gemm.W4_SKINNY == "plan"
    _, mp = small_pair
    L = mp.cfg.num_layers
    _, _, n_pre, n_dec = _prefill_and_decode4(mp)
    assert n_pre["expand_launches"] == 4 * L  # M = 244: above the kernel's 64 rows
    assert n_dec["skinny_launches"] == 3 * L and n_dec["expand_launches"] == L
    m2 = build_model(replace(get_config("small"), name="small3072", intermediate_size=3072), DEV, seed=5,
                     weight_dtype="mxfp4-packed")
    _, _, _, n_dec = _prefill_and_decode4(m2)
    assert n_dec["skinny_launches"] == 4 * L and n_dec["expand_launches"] == 0


# ---- engine -----------------------------------------------------------------------------------------------------------

CHAINS = [["[OPEN] attack_chain.sh -> /tmp/malware.bin", "[EXEC] attack_chain.sh -> curl"],
          ["[EXEC] bash -> chmod", "[OPEN] chmod -> "],
          ["[EXEC] bash -> cat", "[OPEN] cat -> /tmp/malware.bin", "[EXEC] bash -> nc"],
          ["[EXEC] sshd -> bash", "[OPEN] bash -> /etc/shadow"]]


def _engine_texts(weights):
    from chronos.brain.engine.engine import Engine, EngineConfig
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    eng = Engine(EngineConfig(model="small", device="cuda:0", max_slots=4, max_model_len=256, decode_burst=4,
                              weight_dtype=weights))
    assert eng.cfg.use_graphs and eng.model.w.w4
    assert (eng.model.w.layers[0].wqkv.w is None) == (weights == "mxfp4-packed")
    reqs = [eng.submit(build_prompt(c), fmt=VERDICT_SCHEMA, num_predict=40) for c in CHAINS]
    eng.run_until_idle()
    torch.cuda.synchronize()
    for r in reqs:
        assert r.error is None
        assert {"risk_score", "verdict", "reason"} <= set(json.loads(r.text)), r.text
    return [r.text for r in reqs]


def test_packed_engine_with_graphs_equals_copy_mode(dense_route):
    from chronos.ops import gemm

    c0 = gemm.w4_stats["expand_launches"]
    copy = _engine_texts("mxfp4")
    assert gemm.w4_stats["expand_launches"] == c0
    first = _engine_texts("mxfp4-packed")
    assert gemm.w4_stats["expand_launches"] > c0
    second = _engine_texts("mxfp4-packed")
    assert first == second  # the captured expansions replay into the same scratch
    assert first == copy


def test_packed_engine_default_routing():
    from chronos.ops import gemm

    c0 = dict(gemm.w4_stats)
    _engine_texts("mxfp4-packed")  # valid verdicts through the W4A16 kernels and the expansion together
    assert gemm.w4_stats["skinny_launches"] > c0["skinny_launches"]
    assert gemm.w4_stats["expand_launches"] > c0["expand_launches"]


def test_kv_pool_is_no_smaller_than_copy_mode():
    from chronos.brain.engine.engine import Engine, EngineConfig

    blocks = {}
    for weights in ("mxfp4", "mxfp4-packed"):
        eng = Engine(EngineConfig(model="small", device="cuda:0", max_slots=4, max_model_len=256, kv_blocks=0,
                                  weight_dtype=weights))
        blocks[weights] = eng.blocks.num_blocks
        del eng
        torch.cuda.empty_cache()
    assert blocks["mxfp4-packed"] >= blocks["mxfp4"] >= 2, blocks
