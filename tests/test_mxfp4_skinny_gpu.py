"""W4A16 mode of the skinny MFMA GEMM (csrc/kernels/gemm_skinny.hip WM = kW4: OCP MXFP4 weights, bf16 activations,
M <= 64): exact one-hot probes of every position and every code on every config, the dense epilogues (plain, SwiGLU,
the folded norm, the residual producer) against fp32 references on the dequantised copy, split-K determinism, the 8B
shapes, the binding's checks, the routing switch of ops/gemm.py, the mxfp4 model and the engine."""
import json

import pytest
import torch

from _mxfp4_cases import GRID, pack, probe_columns, spread_weight

pytestmark = pytest.mark.gpu
DEV = "cuda"
# W4 cfg -> (RT, MT, NW): csrc/kernels/gemm_skinny.hip SK4_CONFIGS; the unit is 128 k
CFGS = {0: (4, 1, 4), 1: (4, 1, 4), 2: (4, 1, 8), 3: (2, 1, 8), 4: (2, 1, 8), 5: (2, 1, 16), 6: (1, 1, 16),
        7: (4, 2, 4), 8: (2, 2, 8), 9: (4, 2, 8), 10: (4, 4, 4), 11: (2, 4, 8), 12: (2, 4, 4)}
UNIT = 128
EVEN = [c for c in sorted(CFGS) if CFGS[c][0] % 2 == 0]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from chronos import ops
    from chronos.ops import gemm

    ops.load()
    assert gemm._SK4 == CFGS


@pytest.fixture
def switch():
    """Set ops/gemm.py W4_SKINNY for one test; restored afterwards."""
    from chronos.ops import gemm

    old = gemm.W4_SKINNY

    def set_(v):
        gemm.W4_SKINNY = v

    try:
        yield set_
    finally:
        gemm.W4_SKINNY = old


def _q4(w):
    from chronos.models.llama import quantize_mxfp4

    return quantize_mxfp4(w.contiguous())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _sk(x, w4, mode, cfg, splitk=1, resid=None, part=None, eps=1e-5):
    return torch.ops.chronos.gemm_skinny(x, w4.q, mode, cfg, splitk, resid, part, eps, w4.e)


def _rand(shape, g, scale=1.0, shift=0.0):
    return ((torch.rand(shape, device=DEV, generator=g) * 2 - 1) * scale + shift).to(torch.bfloat16)


def _check(y, ref, tol=2e-2):
    """tests/test_gemm_skinny_gpu.py's bound: tol of max |ref|."""
    err = (y.float() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    print(f"max err {err:.4g} vs max |ref| {scale:.4g}")
    assert err <= tol * scale, f"max err {err:.4g} vs max |ref| {scale:.4g}"


def _probe(w4, cols, m, cfg, splitk):
    """y[:, n] for one-hot rows of x at ``cols`` (m rows per launch) -> [len(cols), N] bf16."""
    k = w4.w.shape[1]
    x = torch.zeros(len(cols), k, device=DEV, dtype=torch.bfloat16)
    x[torch.arange(len(cols)), torch.tensor(cols)] = 1.0
    return torch.cat([_sk(x[i:i + m], w4, 0, cfg, splitk)[0] for i in range(0, len(cols), m)])


def _want(w4, cols):
    # one exactly representable term plus zeros; a -0 term and +0 terms sum to +0 (IEEE), so -0 reads back as +0
    return (w4.w[:, torch.tensor(cols, device=DEV)].t().float() + 0.0).to(torch.bfloat16)


# ---- exact probes ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_position_probe(cfg, splitk):
    """Every k lands in the MFMA slot of its x element: one unit per wave, and three so that the ring wraps."""
    rt, mt, nw = CFGS[cfg]
    n = 16 * rt * 3
    for units in (1, 3):
        k = UNIT * nw * splitk * units
        w4 = _q4(spread_weight(n, k, 1000 * cfg + 10 * splitk + units, DEV))
        assert w4.e.min().item() <= 114 and w4.e.max().item() >= 131  # the scales really differ from block to block
        cols = list(range(k)) if k <= 1536 else probe_columns(k, k + cfg)
        want = _bits(_want(w4, cols))
        for m in sorted({1, 3, 16 * mt - 5, 16 * mt}):
            assert torch.equal(_bits(_probe(w4, cols, m, cfg, splitk)), want), (k, m)


def _table_weight(n, k, rows):
    """[n, k] codes / scales: ``rows`` = [(codes of one block [32], e or a per-block e list)], the rest zero at 127."""
    from chronos.models.llama import Q4Tensor
    from chronos.ops import reference as ref

    codes = torch.zeros(n, k // 32, 32, dtype=torch.int32)
    e = torch.full((n, k // 32), 127, dtype=torch.uint8)
    for i, (c, ev) in enumerate(rows):
        codes[i], e[i] = c, ev
    q = pack(codes.reshape(n, k)).to(DEV)
    e = e.to(DEV)
    return Q4Tensor(q, e, ref.dequantize_mxfp4(q, e)), codes, e


@pytest.mark.parametrize("cfg", [3, 4, 11])
def test_code_table_probe(cfg):
    """Every code at the ends of the scale range, in both nibble positions of every block: e = 2 and e = 127 with all
    16 codes, e = 254 with the 8 codes whose value is finite in bf16, and the three scales block by block.  e = 1 is not
    asserted: 0.5 * 2^-126 is a bf16 subnormal, and whether the bf16 MFMA keeps subnormal A inputs is printed below."""
    rt, mt, nw = CFGS[cfg]
    n, k = 16 * rt, UNIT * nw
    nb = k // 32
    all16 = torch.cat([torch.arange(16), torch.arange(15, -1, -1)])  # each code once per nibble position
    fin = torch.tensor([0, 1, 2, 3, 8, 9, 10, 11]).repeat(4)
    fin = torch.cat([fin[:16], fin[16:].flip(0)])
    e3 = torch.tensor([2, 127, 254]).repeat(nb)[:nb].to(torch.uint8)
    c3 = torch.where((e3 == 254)[:, None], fin[None, :], all16[None, :]).to(torch.int32)
    w4, codes, e = _table_weight(n, k, [(all16, 2), (all16, 127), (fin, 254), (c3, e3)])
    assert torch.isfinite(w4.w.float()).all()
    mag = torch.tensor(GRID, dtype=torch.float64)[(codes & 7).long()]
    val = torch.where((codes & 8) != 0, -mag, mag) * torch.exp2(e.cpu().double() - 127)[..., None]
    assert torch.equal(w4.w.cpu().double(), val.reshape(n, k))  # the reference table in exact arithmetic
    cols = list(range(k))
    for m in (1, 16 * mt):
        assert torch.equal(_bits(_probe(w4, cols, m, cfg, 1)), _bits(_want(w4, cols))), m
    # e = 1 (subnormal products), reported only
    ws, _, _ = _table_weight(n, k, [(all16, 1)])
    got, want = _probe(ws, cols[:32], 16 * mt, cfg, 1)[:, 0], _want(ws, cols[:32])[:, 0]
    print("e = 1, row 0, block 0: kernel", got.float().tolist(), "table", want.float().tolist(),
          "equal" if torch.equal(_bits(got), _bits(want)) else "DIFFERENT (subnormals not kept)")


# ---- dense, every epilogue and config ------------------------------------------------------------------------------


def _norm_parts(s, k):
    sf = s.float()
    part = torch.stack([(sf[:, i::8] ** 2).sum(1) for i in range(8)], 1).contiguous()
    return sf, part, torch.rsqrt((sf * sf).sum(1, keepdim=True) / k + 1e-5)


@pytest.mark.parametrize("cfg", sorted(CFGS))
@pytest.mark.parametrize("splitk", [1, 3])
def test_plain_and_normp(cfg, splitk):
    rt, mt, nw = CFGS[cfg]
    g = torch.Generator(device=DEV).manual_seed(7 * cfg + splitk)
    n, k = 512, UNIT * nw * splitk * 2
    w4 = _q4(_rand((n, k), g, 0.5))
    wf = w4.w.float()
    for m in sorted({1, 3, 16 * mt - 5, 16 * mt}):
        s = _rand((m, k), g, 2.0, 0.3)
        sf, part, inv = _norm_parts(s, k)
        _check(_sk(s, w4, 0, cfg, splitk)[0], sf @ wf.t())
        _check(_sk(s, w4, 0, cfg, splitk, None, part)[0], (sf * inv) @ wf.t())


@pytest.mark.parametrize("cfg", EVEN)
@pytest.mark.parametrize("splitk", [1, 2])
def test_swiglu_normp(cfg, splitk):
    rt, mt, nw = CFGS[cfg]
    g = torch.Generator(device=DEV).manual_seed(3 + cfg)
    m, f, k = 16 * mt - 3, 256, UNIT * nw * splitk * 2
    s = _rand((m, k), g, 2.0, 0.3)
    w4 = _q4(_rand((2 * f, k), g, 0.3))
    wf = w4.w.float()
    sf, part, inv = _norm_parts(s, k)
    hv = (sf * inv) @ wf.t()
    _check(_sk(s, w4, 1, cfg, splitk, None, part)[0], torch.nn.functional.silu(hv[:, :f]) * hv[:, f:], 3e-2)
    hp = sf @ wf.t()
    _check(_sk(s, w4, 1, cfg, splitk)[0], torch.nn.functional.silu(hp[:, :f]) * hp[:, f:], 3e-2)


@pytest.mark.parametrize("cfg", sorted(CFGS))
@pytest.mark.parametrize("splitk", [1, 4])
def test_resid_partials(cfg, splitk):
    rt, mt, nw = CFGS[cfg]
    g = torch.Generator(device=DEV).manual_seed(5 + cfg)
    m, n, k = 16 * mt - 2, 512, UNIT * nw * (6 if splitk == 1 else 4)
    x = _rand((m, k), g)
    w4 = _q4(_rand((n, k), g, 0.2))
    r = _rand((m, n), g, 4.0)
    s, part = _sk(x, w4, 2, cfg, splitk, r)
    ref = (x.float() @ w4.w.float().t()).to(torch.bfloat16).float() + r.float()
    _check(s, ref)
    assert part.shape == (m, n // (16 * rt))
    assert torch.allclose(part.sum(1), (s.float() ** 2).sum(1), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_splitk_deterministic(cfg):
    """Split-K sums the slabs in slice order: repeated calls are bitwise equal (a replayed graph == the eager step),
    and the tickets are left at zero by every call."""
    rt, mt, nw = CFGS[cfg]
    g = torch.Generator(device=DEV).manual_seed(40 + cfg)
    m, n, k = 16 * mt - 1, 512, UNIT * nw * 8
    x = _rand((m, k), g)
    w4 = _q4(_rand((n, k), g, 0.5, 0.05))
    first, _ = _sk(x, w4, 0, cfg, 8)
    ref = x.float() @ w4.w.float().t()
    _check(first, ref)
    for _ in range(4):
        assert torch.equal(_sk(x, w4, 0, cfg, 8)[0], first)
    _check(_sk(x, w4, 0, cfg, 1)[0], ref)
    _check(_sk(x, w4, 0, cfg, 1)[0], first.float())


def test_8b_shapes():
    """One call per Llama-3-8B projection at a jump-forward / few-stream M, each on a config valid for it."""
    g = torch.Generator(device=DEV).manual_seed(1)
    for m, n, k, mode, normp, cfg, sk in [(3, 6144, 4096, 0, False, 0, 1), (5, 4096, 14336, 2, False, 3, 2),
                                          (4, 28672, 4096, 1, True, 2, 1), (48, 4096, 4096, 0, False, 10, 2)]:
        x = _rand((m, k), g, 1.0, 0.1)
        w4 = _q4(_rand((n, k), g, 0.05))
        wf = w4.w.float()
        if mode == 2:
            r = _rand((m, n), g, 4.0)
            s, part = _sk(x, w4, 2, cfg, sk, r)
            _check(s, (x.float() @ wf.t()).to(torch.bfloat16).float() + r.float())
            assert torch.allclose(part.sum(1), (s.float() ** 2).sum(1), rtol=1e-4, atol=1e-3)
        elif mode == 1:
            sf, part, inv = _norm_parts(x, k)
            hv = (sf * inv) @ wf.t()
            _check(_sk(x, w4, 1, cfg, sk, None, part)[0],
                   torch.nn.functional.silu(hv[:, :n // 2]) * hv[:, n // 2:], 3e-2)
        else:
            _check(_sk(x, w4, 0, cfg, sk)[0], x.float() @ wf.t())


def test_binding_checks():
    g = torch.Generator(device=DEV).manual_seed(2)
    k = UNIT * 8  # cfg 3: RT 2, MT 1, NW 8
    x = _rand((20, k), g)
    w4 = _q4(_rand((256, k), g))
    op = torch.ops.chronos.gemm_skinny
    y, _ = op(x[:8], w4.q, 0, 3, 1, None, None, 1e-5, w4.e)
    _check(y, x[:8].float() @ w4.w.float().t())
    with pytest.raises(RuntimeError):
        op(x[:8], w4.q, 0, 3, 1, None, None, 1e-5, w4.e[:, :16].contiguous())  # we is not [N, K / 32]
    with pytest.raises(RuntimeError):
        op(x[:8], w4.w, 0, 3, 1, None, None, 1e-5, w4.e)                       # bf16 w with we
    with pytest.raises(RuntimeError):
        op(x[:8], w4.q, 0, len(CFGS), 1, None, None, 1e-5, w4.e)               # W4 config id out of range
    with pytest.raises(RuntimeError):
        op(x[:8], w4.q, 0, 3, 2, None, None, 1e-5, w4.e)                       # K % (128 * NW * splitk)
    with pytest.raises(RuntimeError):
        op(x[:8], w4.q, 0, 5, 1, None, None, 1e-5, w4.e)                       # cfg 5: NW 16, K % 2048
    with pytest.raises(RuntimeError):
        op(x, w4.q, 0, 3, 1, None, None, 1e-5, w4.e)                           # M = 20 > 16 MT
    x16 = _rand((8, 2048), g)
    w16 = _q4(_rand((256, 2048), g))
    with pytest.raises(RuntimeError):
        op(x16, w16.q, 1, 6, 1, None, None, 1e-5, w16.e)                       # SwiGLU on an odd RT (cfg 6)
    r = _rand((8, 256), g)
    part = torch.ones(8, 8, device=DEV)
    with pytest.raises(RuntimeError):
        op(x[:8], w4.q, 2, 3, 1, r, part, 1e-5, w4.e)                          # resid with part_in
    y2, _ = op(x[:8], w4.w, 0, 1, 1, None, None, 1e-5)                         # the 8-argument bf16 call still works
    _check(y2, x[:8].float() @ w4.w.float().t())


# ---- routing -----------------------------------------------------------------------------------------------------


def _wx(m, n, k, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(m, k, device=DEV, generator=g) + 0.1).to(torch.bfloat16)
    return x, _q4((torch.randn(n, k, device=DEV, generator=g) * 0.02).to(torch.bfloat16)), g


def test_routing_switch(switch):
    from chronos import ops
    from chronos.ops import gemm
    from chronos.ops.gemm import LazyNorm

    m, n, k = 4, 512, 1024  # no "w4plans" row
    x, w4, g = _wx(m, n, k, 2)
    wf = w4.w.float()
    xr = (torch.randn(m, n, device=DEV, generator=g) + 0.1).to(torch.bfloat16)
    wd = _q4((torch.randn(k, n, device=DEV, generator=g) * 0.02).to(torch.bfloat16))  # [N = 1024, K = 512]
    sf, part, inv = _norm_parts(x, k)
    lazy = lambda: LazyNorm(x, part, torch.ones(k, device=DEV, dtype=torch.bfloat16), 1e-5)  # noqa: E731
    count = lambda: gemm.w4_stats["skinny_launches"]  # noqa: E731

    for mode in ("plan", "off"):
        switch(mode)
        c0 = count()
        assert gemm.w4_plan(m, n, k) is None
        assert torch.equal(ops.linear(x, w4), ops.linear(x, w4.w))
        assert torch.equal(ops.gate_up_silu(x, w4), ops.gate_up_silu(x, w4.w))
        assert count() == c0

    switch("model")
    c0 = count()
    _check(ops.linear(x, w4), x.float() @ wf.t())
    assert count() == c0 + 1
    hp = x.float() @ wf.t()
    _check(ops.gate_up_silu(x, w4), torch.nn.functional.silu(hp[:, :n // 2]) * hp[:, n // 2:], 3e-2)
    assert count() == c0 + 2
    hv = (sf * inv) @ wf.t()
    _check(ops.gate_up_silu(lazy(), w4), torch.nn.functional.silu(hv[:, :n // 2]) * hv[:, n // 2:], 3e-2)
    assert count() == c0 + 3
    _check(ops.linear(lazy(), w4), hv)
    assert count() == c0 + 4
    resid = torch.randn(m, k, device=DEV, generator=g).to(torch.bfloat16)
    out = ops.gemv_resid(xr, wd, resid)
    assert count() == c0 + 5 and out.part.shape[0] == m and out.s.shape == resid.shape
    _check(out.s, (xr.float() @ wd.w.float().t()).to(torch.bfloat16).float() + resid.float())
    assert torch.allclose(out.part.sum(1), (out.s.float() ** 2).sum(1), rtol=1e-4, atol=1e-3)
    gemm._W4A16_DECODE = False  # CHRONOS_W4A16_DECODE=0 still forces the copy everywhere
    try:
        assert torch.equal(ops.linear(x, w4), ops.linear(x, w4.w))
        assert count() == c0 + 5
    finally:
        gemm._W4A16_DECODE = True
    switch("off")
    assert torch.equal(ops.linear(x, w4), ops.linear(x, w4.w)) and count() == c0 + 5


# ---- model and engine --------------------------------------------------------------------------------------------


def test_mxfp4_model_skinny_vs_bf16_copy(switch):
    from chronos.models.llama import KVCache, StepBatch, build_model, make_prefill_batch
    from chronos.ops import gemm

    m = build_model("small", DEV, seed=5, weight_dtype="mxfp4")
    assert m.w.w4
    prompts = [list(range(100 + 7 * b, 161 + 7 * b)) for b in range(4)]
    bts = [list(range(1 + 5 * b, 6 + 5 * b)) for b in range(4)]
    it = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    res, launches = {}, {}
    for name in ("model", "off"):
        switch(name)
        kv = KVCache(m.cfg, m.tp, 32, 16, DEV)
        m.forward(make_prefill_batch(prompts, [0] * 4, bts, m.cfg, m.tp, DEV, max_blocks=8, nqt=8), kv)
        bt_t = torch.zeros(4, 8, dtype=torch.int32, device=DEV)
        for b in range(4):
            bt_t[b, :5] = it(bts[b])
        dec = StepBatch(it([777, 778, 779, 780]), it([61] * 4), it([0, 1, 2, 3]), bt_t, it([0, 1, 2, 3, 4]),
                        it([62] * 4), torch.arange(4, dtype=torch.int64, device=DEV), None, 4)
        c0 = gemm.w4_stats["skinny_launches"]
        res[name] = m.forward(dec, kv).float()
        c1 = gemm.w4_stats["skinny_launches"]
        jf = make_prefill_batch([[5, 6, 7]], [62], [bts[0]], m.cfg, m.tp, DEV, max_blocks=8, nqt=2)
        res[name + "_jf"] = m.forward(jf, kv).float()
        launches[name] = (c1 - c0, gemm.w4_stats["skinny_launches"] - c1)
    L = m.cfg.num_layers
    # small: QKV, O and gate_up have K = 1024; down has K = 2816 = 128 * 22, which no config's wave count divides
    assert min(launches["model"]) >= 2 * L and launches["off"] == (0, 0), launches
    cos = lambda a, b: torch.nn.functional.cosine_similarity(a, b, dim=-1).min().item()  # noqa: E731
    print("min cosine", cos(res["model"], res["off"]), cos(res["model_jf"], res["off_jf"]), launches)
    assert cos(res["model"], res["off"]) > 0.995
    assert cos(res["model_jf"], res["off_jf"]) > 0.995


def test_mxfp4_engine_skinny(switch):
    from chronos.brain.engine.engine import Engine, EngineConfig
    from chronos.ops import gemm
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    chains = [["[OPEN] attack_chain.sh -> /tmp/malware.bin", "[EXEC] attack_chain.sh -> curl"],
              ["[EXEC] bash -> chmod", "[OPEN] chmod -> "],
              ["[EXEC] bash -> cat", "[OPEN] cat -> /tmp/malware.bin", "[EXEC] bash -> nc"],
              ["[EXEC] sshd -> bash", "[OPEN] bash -> /etc/shadow"]]
    switch("model")
    texts = []
    for _ in range(2):
        eng = Engine(EngineConfig(model="small", device="cuda:0", max_slots=4, max_model_len=256, decode_burst=4,
                                  weight_dtype="mxfp4"))
        assert eng.cfg.use_graphs and eng.model.w.w4
        before = gemm.w4_stats["skinny_launches"]
        reqs = [eng.submit(build_prompt(c), fmt=VERDICT_SCHEMA, num_predict=40) for c in chains]
        eng.run_until_idle()
        torch.cuda.synchronize()
        for r in reqs:
            assert r.error is None
            assert {"risk_score", "verdict", "reason"} <= set(json.loads(r.text)), r.text
        assert gemm.w4_stats["skinny_launches"] > before
        texts.append([r.text for r in reqs])
        del eng
    assert texts[0] == texts[1]  # graph replay and the split-K order are stable
