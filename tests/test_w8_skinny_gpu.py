"""W8A16 mode of the skinny MFMA GEMM (csrc/kernels/gemm_skinny.hip WM = kW8: e4m3 weights with per-row f32 scales, bf16
activations, M <= 64): exact integer probes of every config, split-K and epilogue, the whole e4m3 code table at every
byte position of a lane's piece, random operands against fp32 on the dequantised weight, split-K determinism, the
binding's checks, the opt-in routing of ops/gemm.py, the fp8 model above two rows and the engine.

Exactness of the integer probes (tests/_gemm_probes.py builders): x in {-2..2}, W a signed permutation per G x G block
stored as e4m3 +-1 (exact), so x W^T is an integer with |.| <= 128; the row scales are 1 or 2, so the scaled sum is an
integer <= 256 in magnitude, exact in fp32 in any order and exact in bf16.  With the integer residual (|r| <= 64)
s = bf16(bf16(y) + r) is one correct rounding of an exact integer sum (<= 320: an integer again), and a partial is a sum
of at most 64 squares of integers <= 320, below 2^23: exact in fp32 in any order.  SwiGLU gates are |g| <= 64 and the
folded-norm scale is a power of two up to 1e-6, which is what that file's 2^-7 bound is derived for."""
import json

import pytest
import torch

import _gemm_probes as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
# W8 cfg -> (RT, MT, NW) and the ring depth D in 64-k units: csrc/kernels/gemm_skinny.hip SK8_CONFIGS
CFGS = {0: (4, 1, 4), 1: (4, 1, 8), 2: (2, 1, 8), 3: (2, 1, 16), 4: (1, 1, 16), 5: (4, 2, 4), 6: (2, 2, 8),
        7: (4, 2, 8), 8: (4, 4, 4), 9: (2, 4, 8), 10: (2, 4, 4), 11: (1, 1, 8)}
DEPTH = {0: 8, 1: 6, 2: 8, 3: 4, 4: 8, 5: 6, 6: 8, 7: 4, 8: 4, 9: 4, 10: 6, 11: 8}
UNIT = 64
SMALL = ((1536, 1024, 0), (1024, 1024, 2), (5632, 1024, 1), (1024, 2816, 2))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from chronos import ops
    from chronos.ops import gemm

    ops.load()
    assert gemm._SK8 == CFGS


@pytest.fixture
def switch():
    """Set ops/gemm.py W8_SKINNY for one test; restored afterwards."""
    from chronos.ops import gemm

    old = gemm.W8_SKINNY

    def set_(v):
        gemm.W8_SKINNY = v

    try:
        yield set_
    finally:
        gemm.W8_SKINNY = old


def _sk(x, wq, ws, mode, cfg, splitk=1, resid=None, part=None, eps=P.EPS):
    return torch.ops.chronos.gemm_skinny(x, wq, mode, cfg, splitk, resid, part, eps, None, ws)


def _row_scales(n, seed):
    """f32 [n] of 1 and 2, seeded, never three equal in a row."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    s = torch.randint(0, 2, (n,), generator=g, device=DEV)
    s[2::3] = 1 - s[1::3][:s[2::3].numel()]
    return torch.pow(2.0, s.float())


# ---- exact integer probes ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("splitk", [1, 2, 3])
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_integer_probe(cfg, splitk):
    rt, mt, nw = CFGS[cfg]
    n, k = 32 * rt, UNIT * nw * splitk * (DEPTH[cfg] + 2)  # prologue, steady ring and refill are all crossed
    bad = []
    for m in sorted({1, 3, 16 * mt - 1, 16 * mt}):
        seed = 1000 * cfg + 100 * splitk + m
        x = P.carve(P.make_x(m, k, seed, DEV))
        w = P.make_w(n, k, seed + 1, DEV)
        ws = P.carve(_row_scales(n, seed + 2))
        wq = P.carve(P.to_e4m3(w))
        h = P.expect_plain(x, w) * ws.double()[None, :]
        assert h.abs().max().item() <= 256
        y = _sk(x, wq, ws, 0, cfg, splitk)[0]
        if not torch.equal(y, h.to(torch.bfloat16)):
            bad.append(("plain", m, int((y.double() != h).sum())))
        # the residual producer and its partials
        r = P.carve(P.make_resid(m, n, seed + 3, DEV))
        s, part = _sk(x, wq, ws, 2, cfg, splitk, r)
        want = (h + r.double()).to(torch.bfloat16)
        if not torch.equal(s, want):
            bad.append(("resid", m, int((s != want).sum())))
        # every partial by itself: entry [m, g] is the sum of s^2 over the 16 RT columns of workgroup g
        want_part = (want.double() ** 2).view(m, n // (16 * rt), 16 * rt).sum(2)
        if part.shape != want_part.shape or not torch.equal(part.double(), want_part):
            bad.append(("partials", m, tuple(part.shape)))
        # the folded norm as a row scale
        pin = P.carve(P.make_parts(m, k, 8, seed + 4, DEV))
        inv = P.inv_of(pin, k)
        y = _sk(x, wq, ws, 0, cfg, splitk, None, pin)[0]
        if not bool(P.close(y, h * inv).all()):
            bad.append(("normp", m, int((~P.close(y, h * inv)).sum())))
        if rt % 2 == 0:
            wg = P.make_w_swiglu(n // 2, k, seed + 5, DEV)
            wgq = P.carve(P.to_e4m3(wg))
            hg = P.expect_plain(x, wg) * ws.double()[None, :]
            f = n // 2
            assert hg[:, :f].abs().max().item() <= 64
            for tag, sc, pi in (("swiglu", 1.0, None), ("swiglu+normp", inv, pin)):
                g_, u_ = hg[:, :f] * sc, hg[:, f:] * sc
                e = g_ / (1.0 + torch.exp(-g_)) * u_
                y = _sk(x, wgq, ws, 1, cfg, splitk, None, pi)[0]
                if y.shape != e.shape or not bool(P.close(y, e).all()):
                    bad.append((tag, m, int((~P.close(y, e)).sum())))
    torch.cuda.synchronize()
    assert not bad, bad


def test_swiglu_on_an_odd_rt_is_refused():
    odd = [c for c in CFGS if CFGS[c][0] % 2]
    assert odd
    for cfg in odd:
        rt, mt, nw = CFGS[cfg]
        k = UNIT * nw
        x = torch.zeros(1, k, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            _sk(x, torch.zeros(64, k, device=DEV, dtype=torch.uint8), torch.ones(64, device=DEV), 1, cfg)


# ---- the code table ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_code_table_probe(cfg):
    """All 254 non-NaN e4m3fn bytes, subnormals and both zeros included, at each of the 16 byte positions of a lane's
    piece, read back through a one-hot x: y == value * scale exactly (e4m3 has 4 significant bits, the scales are
    powers of two, every other term of the sum is a zero)."""
    rt, mt, nw = CFGS[cfg]
    n, k = 16 * rt, UNIT * nw
    codes = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.int64)
    assert codes.numel() == 254
    nn, kk = torch.meshgrid(torch.arange(n), torch.arange(k), indexing="ij")
    slot = nn * (k // 16) + kk // 16  # >= 256 consecutive slots per byte position
    idx = (slot + 31 * (kk % 16)) % 254
    for p in range(16):
        assert idx[kk % 16 == p].unique().numel() == 254
    wq = P.carve(codes[idx].to(torch.uint8).to(DEV))
    ws = P.carve(torch.pow(2.0, (torch.arange(n, device=DEV) % 5 - 2).float()))
    val = wq.view(torch.float8_e4m3fn).double()
    assert bool(val.isfinite().all()) and val.abs().min().item() == 0 and val.abs().max().item() == 448
    assert (val.abs()[val != 0].min().item()) == 2.0 ** -9  # the smallest subnormal is in the table
    want = (val * ws.double()[:, None]).t()  # [K, N]: row j = the output of one-hot column j
    assert torch.equal(want.to(torch.bfloat16).double(), want)
    eye = torch.eye(k, device=DEV, dtype=torch.bfloat16)
    for m in (1, 16 * mt):
        cols = range(0, k, m) if m > 1 else range(0, k, 7)
        for j in cols:
            x = P.carve(eye[j:j + m])
            y = _sk(x, wq, ws, 0, cfg)[0]
            assert torch.equal(y.double(), want[j:j + m]), (m, j)


# ---- random operands -----------------------------------------------------------------------------------------------


def _deq(q, s):
    return q.view(torch.float8_e4m3fn).float() * s.float()[:, None]


def _wx(m, n, k, seed):
    from chronos.ops import reference as ref

    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(m, k, device=DEV, generator=g) + 0.1).to(torch.bfloat16)
    w = (torch.randn(n, k, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    wq, ws = ref.quantize_weight(w)
    return x, wq.contiguous(), ws.contiguous(), g


def _close(y, want):
    """tests/test_w8a16_gpu.py's bound."""
    err = (y.float() - want.float()).abs().max().item()
    print(f"max err {err:.4g} vs max |ref| {want.float().abs().max().item():.4g}")
    assert err <= 1e-2 * want.float().abs().max().item() + 1e-3, (err, want.float().abs().max().item())


def _swiglu_ref(full, n):
    gt, up = full[:, :n // 2].bfloat16().float(), full[:, n // 2:].bfloat16().float()
    return (gt / (1 + torch.exp(-gt))).bfloat16().float() * up


def _norm_parts(s, k):
    sf = s.float()
    part = torch.stack([(sf[:, i::8] ** 2).sum(1) for i in range(8)], 1).contiguous()
    return sf, part, torch.rsqrt((sf * sf).sum(1, keepdim=True) / k + 1e-5)


@pytest.mark.parametrize("m", [3, 17, 64])
@pytest.mark.parametrize("n,k,mode", SMALL + ((6144, 4096, 0), (4096, 14336, 2), (28672, 4096, 1)))
def test_random_operands(m, n, k, mode):
    """Every epilogue the model uses on the shape (the folded norm included) on the cost-model's config."""
    from chronos.ops import gemm

    pick = gemm._sk8_model(m, n, k, mode)
    assert pick is not None, "no W8 config accepts this shape"
    cfg, sk = pick
    x, wq, ws, g = _wx(m, n, k, 13 * n + k + m)
    wf = _deq(wq, ws)
    if mode == 2:
        r = torch.randn(m, n, device=DEV, generator=g).to(torch.bfloat16)
        s, part = _sk(x, wq, ws, 2, cfg, sk, r)
        _close(s, (x.float() @ wf.t()).bfloat16().float() + r.float())
        torch.testing.assert_close(part.sum(1), (s.float() ** 2).sum(1), rtol=1e-3, atol=1e-2)
        return
    sf, part, inv = _norm_parts(x, k)
    for pin, xin in ((None, sf), (part, sf * inv)):
        full = xin @ wf.t()
        _close(_sk(x, wq, ws, mode, cfg, sk, None, pin)[0], _swiglu_ref(full, n) if mode == 1 else full)


# ---- split-K -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_splitk_repeats_and_aba(cfg):
    """Split-K sums the slabs in slice order and leaves its tickets at zero: repeats are bitwise equal, and operands A,
    B, A through the same workspace give A's bits again (a stale slab or ticket would show in the call after it)."""
    rt, mt, nw = CFGS[cfg]
    m, n, k = 16 * mt - 1, 32 * rt, UNIT * nw * 4 * 3
    xa, wqa, wsa, g = _wx(m, n, k, 40 + cfg)
    xb, wqb, wsb, _ = _wx(m, n, k, 90 + cfg)
    ra = torch.randn(m, n, device=DEV, generator=g).to(torch.bfloat16)
    first = _sk(xa, wqa, wsa, 0, cfg, 4)[0]
    _close(first, xa.float() @ _deq(wqa, wsa).t())
    for _ in range(3):
        assert torch.equal(_sk(xa, wqa, wsa, 0, cfg, 4)[0], first)
    sa, pa = _sk(xa, wqa, wsa, 2, cfg, 4, ra)
    yb = _sk(xb, wqb, wsb, 0, cfg, 4)[0]
    _close(yb, xb.float() @ _deq(wqb, wsb).t())
    assert torch.equal(_sk(xa, wqa, wsa, 0, cfg, 4)[0], first)
    sa2, pa2 = _sk(xa, wqa, wsa, 2, cfg, 4, ra)
    assert torch.equal(sa, sa2) and torch.equal(pa, pa2)
    _close(_sk(xa, wqa, wsa, 0, cfg, 1)[0], first)


# ---- the binding ---------------------------------------------------------------------------------------------------


def test_binding_checks():
    k = UNIT * 8  # cfg 2: RT 2, MT 1, NW 8
    x, wq, ws, g = _wx(20, 256, k, 2)
    op = torch.ops.chronos.gemm_skinny
    y, _ = op(x[:8], wq, 0, 2, 1, None, None, 1e-5, None, ws)
    _close(y, x[:8].float() @ _deq(wq, ws).t())
    e = torch.zeros(256, k // 32, device=DEV, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        op(x[:8], wq, 0, 2, 1, None, None, 1e-5, e, ws)                              # we and wscale together
    with pytest.raises(RuntimeError):
        op(x[:8], wq.view(torch.float8_e4m3fn).to(torch.bfloat16), 0, 2, 1, None, None, 1e-5, None, ws)  # bf16 w
    with pytest.raises(RuntimeError):
        op(x[:8], wq, 0, 2, 1, None, None, 1e-5, None, ws[:128].contiguous())        # wscale is not [N]
    with pytest.raises(RuntimeError):
        op(x[:8], wq, 0, 2, 1, None, None, 1e-5, None, ws.double())                  # wscale is not f32
    with pytest.raises(RuntimeError):
        op(x[:8], wq[:, :k - 64], 0, 2, 1, None, None, 1e-5, None, ws)               # w is not contiguous [N, K]
    off = torch.empty(256 * k + 1, device=DEV, dtype=torch.uint8)[1:].view(256, k)
    with pytest.raises(RuntimeError):
        op(x[:8], off, 0, 2, 1, None, None, 1e-5, None, ws)                          # w is not 16-B aligned
    with pytest.raises(RuntimeError):
        op(x[:8], wq, 0, len(CFGS), 1, None, None, 1e-5, None, ws)                   # W8 config id out of range
    with pytest.raises(RuntimeError):
        op(x[:8], wq, 0, 2, 2, None, None, 1e-5, None, ws)                           # K % (64 * NW * splitk)
    with pytest.raises(RuntimeError):
        op(x[:8], wq, 0, 3, 1, None, None, 1e-5, None, ws)                           # cfg 3: NW 16, K % 1024
    with pytest.raises(RuntimeError):
        op(x, wq, 0, 2, 1, None, None, 1e-5, None, ws)                               # M = 20 > 16 MT
    with pytest.raises(RuntimeError):
        op(x[:8], wq[:240].contiguous(), 0, 0, 1, None, None, 1e-5, None, ws[:240].contiguous())  # N % (16 RT), cfg 0
    r = torch.zeros(8, 256, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        op(x[:8], wq, 2, 2, 1, r, torch.ones(8, 8, device=DEV), 1e-5, None, ws)      # resid with part_in
    with pytest.raises(RuntimeError):
        op(x[:8], wq.cpu(), 0, 2, 1, None, None, 1e-5, None, ws)                     # w on the host
    wb = _deq(wq, ws).to(torch.bfloat16)
    y2, _ = op(x[:8], wb, 0, 1, 1, None, None, 1e-5)                                 # the 8-argument bf16 call still works
    _close(y2, x[:8].float() @ wb.float().t())


# ---- routing -------------------------------------------------------------------------------------------------------


def test_routing_switch(switch):
    from chronos import ops
    from chronos.models.llama import QTensor
    from chronos.ops import gemm
    from chronos.ops.gemm import LazyNorm

    m, n, k = 5, 512, 1024  # no "w8plans" row
    x, wq, ws, g = _wx(m, n, k, 2)
    w8 = QTensor(wq, ws)
    wf = _deq(wq, ws)
    xd, wqd, wsd, _ = _wx(m, k, n, 3)  # the producer: [N = 1024, K = 512]
    wd = QTensor(wqd, wsd)
    resid = torch.randn(m, k, device=DEV, generator=g).to(torch.bfloat16)
    sf, part, inv = _norm_parts(x, k)
    lazy = lambda: LazyNorm(x, part, torch.ones(k, device=DEV, dtype=torch.bfloat16), 1e-5)  # noqa: E731
    count = lambda: gemm.w8_stats["skinny_launches"]  # noqa: E731

    switch("off")
    today = (ops.linear(x, w8), ops.gate_up_silu(x, w8), ops.linear(lazy(), w8))
    for mode in ("off", "plan", "model"):
        switch(mode)
        c0 = count()
        assert not ops.resid_ok(m, k, n, True)
        if mode != "model":
            assert gemm.w8_plan(m, n, k) is None and not ops.resid_ok_a16(m, k, n)
            assert not ops.w8a16_step_ok(m, ((n, k, 0), (k, n, 2)))
            a16 = (ops.linear(x, w8, a16=True), ops.gate_up_silu(x, w8, a16=True), ops.linear(lazy(), w8, a16=True))
            assert all(torch.equal(a, b) for a, b in zip(a16, today))
        # default calls never reach the kernel, whatever the switch says
        now = (ops.linear(x, w8), ops.gate_up_silu(x, w8), ops.linear(lazy(), w8))
        assert all(torch.equal(a, b) for a, b in zip(now, today))
        assert count() == c0

    switch("model")
    c0 = count()
    assert ops.w8a16_step_ok(m, ((n, k, 0), (k, n, 2), (n, k, 1)))
    _close(ops.linear(x, w8, a16=True), x.float() @ wf.t())
    assert count() == c0 + 1
    _close(ops.gate_up_silu(x, w8, a16=True), _swiglu_ref(x.float() @ wf.t(), n))
    assert count() == c0 + 2
    _close(ops.gate_up_silu(lazy(), w8, a16=True), _swiglu_ref((sf * inv) @ wf.t(), n))
    _close(ops.linear(lazy(), w8, a16=True), (sf * inv) @ wf.t())
    assert count() == c0 + 4
    assert ops.resid_ok_a16(m, k, n)
    out = ops.gemv_resid(xd, wd, resid, a16=True)
    assert count() == c0 + 5 and out.s.shape == resid.shape and out.part.shape[0] == m
    _close(out.s, (xd.float() @ _deq(wqd, wsd).t()).bfloat16().float() + resid.float())
    torch.testing.assert_close(out.part.sum(1), (out.s.float() ** 2).sum(1), rtol=1e-3, atol=1e-2)
    # two rows stay on the W8A16 GEMV, which takes this shape
    y2 = ops.linear(x[:2], w8, a16=True)
    assert count() == c0 + 5 and torch.equal(y2, ops.linear(x[:2], w8))


# ---- model and engine ----------------------------------------------------------------------------------------------


def _model_steps(m, kvmod):
    """Logits of a 3-token chunk, a 5-row and a 33-row decode step after a short prefill."""
    KVCache, StepBatch, make_prefill_batch = kvmod
    it = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    nseq = 33
    prompts = [list(range(100 + 3 * b, 117 + 3 * b)) for b in range(nseq)]  # 17 tokens: two blocks of 16 each
    bts = [[1 + 2 * b, 2 + 2 * b] for b in range(nseq)]
    kv = KVCache(m.cfg, m.tp, 2 * nseq + 2, 16, DEV)
    m.forward(make_prefill_batch(prompts, [0] * nseq, bts, m.cfg, m.tp, DEV, max_blocks=4, nqt=8), kv)
    out = {}
    for rows in (5, 33):
        bt_t = torch.zeros(rows, 4, dtype=torch.int32, device=DEV)
        for b in range(rows):
            bt_t[b, :2] = it(bts[b])
        dec = StepBatch(it([700 + b for b in range(rows)]), it([17] * rows), it(list(range(rows))), bt_t,
                        it(list(range(rows + 1))), it([18] * rows), torch.arange(rows, dtype=torch.int64, device=DEV),
                        None, rows)
        out[f"dec{rows}"] = m.forward(dec, kv).float()
    jf = make_prefill_batch([[5, 6, 7]], [18], [bts[0]], m.cfg, m.tp, DEV, max_blocks=4, nqt=2)
    out["jf3"] = m.forward(jf, kv).float()
    return out


def test_fp8_model_above_two_rows(switch):
    from chronos.models import llama
    from chronos.models.llama import KVCache, StepBatch, build_model, make_prefill_batch
    from chronos.ops import gemm

    kvmod = (KVCache, StepBatch, make_prefill_batch)
    mb = build_model("small", DEV, seed=5)
    mq = build_model("small", DEV, seed=5, weight_dtype="fp8")
    assert mq.w8a16_rows == 2
    count = lambda: gemm.w8_stats["skinny_launches"]  # noqa: E731
    switch("model")
    res = {"bf16": _model_steps(mb, kvmod)}
    c0 = count()
    res["rows2"] = _model_steps(mq, kvmod)  # the default bound: nothing above two rows changes
    assert count() == c0
    llama._W8A16_DECODE = False
    try:
        res["w8a8"] = _model_steps(mq, kvmod)
        mq.w8a16_rows = 64
        res["forced"] = _model_steps(mq, kvmod)  # the flag still forces W8A8 everywhere
        assert count() == c0
    finally:
        llama._W8A16_DECODE = True
    switch("off")
    res["off64"] = _model_steps(mq, kvmod)  # rows = 64 without a route: wholly W8A8
    assert count() == c0
    switch("model")
    res["a16"] = _model_steps(mq, kvmod)
    L = mq.cfg.num_layers
    assert count() - c0 == 3 * 4 * L, (count() - c0, L)  # four projections per layer in each of the three steps
    cos = lambda a, b: torch.nn.functional.cosine_similarity(a, b, dim=-1).min().item()  # noqa: E731
    for step in ("jf3", "dec5", "dec33"):
        assert torch.equal(res["rows2"][step], res["w8a8"][step]), step   # rows = 2: the parent's route, bit for bit
        assert torch.equal(res["forced"][step], res["w8a8"][step]), step
        assert torch.equal(res["off64"][step], res["w8a8"][step]), step
        c8, cb = cos(res["a16"][step], res["w8a8"][step]), cos(res["a16"][step], res["bf16"][step])
        print(step, "min cosine vs W8A8", c8, "vs bf16", cb)
        assert c8 > 0.995 and cb > 0.98, (step, c8, cb)


def test_fp8_engine_a16_rows(switch):
    from chronos.brain.engine.engine import Engine, EngineConfig
    from chronos.ops import gemm
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    chains = [["[OPEN] attack_chain.sh -> /tmp/malware.bin", "[EXEC] attack_chain.sh -> curl"],
              ["[EXEC] bash -> chmod", "[OPEN] chmod -> "],
              ["[EXEC] bash -> cat", "[OPEN] cat -> /tmp/malware.bin", "[EXEC] bash -> nc"],
              ["[EXEC] sshd -> bash", "[OPEN] bash -> /etc/shadow"],
              ["[EXEC] cron -> sh", "[OPEN] sh -> /tmp/.x", "[EXEC] sh -> wget"]]
    switch("model")
    with pytest.raises(ValueError):
        Engine(EngineConfig(model="small", device="cuda:0", weight_dtype="fp8", fp8_a16_rows=65))
    eng = Engine(EngineConfig(model="small", device="cuda:0", max_slots=8, max_model_len=256, decode_burst=4,
                              weight_dtype="fp8", fp8_a16_rows=64))
    assert eng.cfg.use_graphs and eng.model.w.fp8 and eng.model.w8a16_rows == 64
    before = gemm.w8_stats["skinny_launches"]
    reqs = [eng.submit(build_prompt(c), fmt=VERDICT_SCHEMA, num_predict=40) for c in chains]
    eng.run_until_idle()
    torch.cuda.synchronize()
    for r in reqs:
        assert r.error is None
        assert {"risk_score", "verdict", "reason"} <= set(json.loads(r.text)), r.text
    assert gemm.w8_stats["skinny_launches"] > before
