"""Mid-M W4A16 GEMM (csrc/kernels/gemm_w4m.hip: OCP MXFP4 weights, bf16 activations, routed for M = 65-512) on the GPU:
exact one-hot probes of every position and every code, the exact integer probes of tests/_w4m_probes.py through every
config, ring depth, split-K, row count and epilogue (operands carved into poison), split-K determinism with the tickets
read back, the 8B shapes with random data, the binding's checks, the routing switch of ops/gemm.py, the mxfp4 model in
both weight modes and the engine.

Bounds.  Position / code probes: the bits.  Integer probes: plain, residual and the residual's partials by equality
(every partial sum is an integer below 2^24), the ``frac`` residual's partials within ``_gemm_probes.part_bound`` of the
stored values' squares, SwiGLU and the norm prologue within ``_gemm_probes.close`` (2^-7, derived there).  Random data:
the project's 2e-2 (SwiGLU 3e-2) of max |ref| against fp32 on the dequantised copy."""
import json

import pytest
import torch

import _gemm_probes as P
import _w4m_probes as W
from _mxfp4_cases import GRID, pack, spread_weight

pytestmark = pytest.mark.gpu
DEV = "cuda"
# cfg -> (WN, XM, ST): csrc/kernels/gemm_w4m.hip W4M_CONFIGS; a stage is 128 k
CFGS = {0: (64, 64, 4), 1: (128, 64, 4), 2: (64, 128, 4), 3: (128, 128, 4)}
STAGE = 128


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from chronos import ops
    from chronos.ops import gemm

    ops.load()
    assert gemm._W4M == CFGS


@pytest.fixture
def switch():
    """Set ops/gemm.py W4_MID for one test; restored afterwards."""
    from chronos.ops import gemm

    old = gemm.W4_MID

    def set_(v):
        gemm.W4_MID = v

    try:
        yield set_
    finally:
        gemm.W4_MID = old


def test_python_table_is_the_kernels():
    tab = torch.ops.chronos.gemm_w4m_configs()
    assert tab.device.type == "cpu" and tab.shape == (len(CFGS), 3)
    assert {i: tuple(r) for i, r in enumerate(tab.tolist())} == CFGS
    assert len(CFGS) <= 8


def _q4(w):
    from chronos.models.llama import quantize_mxfp4

    return quantize_mxfp4(w.contiguous())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _op(x, q, e, mode, cfg, splitk=1, resid=None, part=None, eps=P.EPS):
    return torch.ops.chronos.gemm_w4m(x, q, e, mode, cfg, splitk, resid, part, eps)


def _rand(shape, g, scale=1.0, shift=0.0):
    return ((torch.rand(shape, device=DEV, generator=g) * 2 - 1) * scale + shift).to(torch.bfloat16)


def _check(y, ref, tol=2e-2):
    err = (y.float() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    print(f"max err {err:.4g} vs max |ref| {scale:.4g}")
    assert err <= tol * scale, f"max err {err:.4g} vs max |ref| {scale:.4g}"


# ---- one-hot probes ------------------------------------------------------------------------------------------------


def _probe(w4, cols, m, cfg, splitk):
    """y[:, n] for one-hot rows of x at ``cols`` (m rows per launch) -> [len(cols), N] bf16."""
    k = w4.w.shape[1]
    x = torch.zeros(len(cols), k, device=DEV, dtype=torch.bfloat16)
    x[torch.arange(len(cols)), torch.tensor(cols)] = 1.0
    return torch.cat([_op(x[i:i + m], w4.q, w4.e, 0, cfg, splitk)[0] for i in range(0, len(cols), m)])


def _want(w4, cols):
    # one exactly representable term plus zeros; a -0 term and +0 terms sum to +0 (IEEE), so -0 reads back as +0
    return (w4.w[:, torch.tensor(cols, device=DEV)].t().float() + 0.0).to(torch.bfloat16)


@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_position_probe(cfg, splitk):
    """Every k lands in the MFMA slot of its x element: one stage per slice, a ring that never fills, one that wraps."""
    wn, xm, st = CFGS[cfg]
    n = 3 * wn
    for stages in sorted({1, st - 1, st + 2}):
        k = STAGE * stages * splitk
        w4 = _q4(spread_weight(n, k, 1000 * cfg + 10 * splitk + stages, DEV))
        assert w4.e.min().item() <= 114 and w4.e.max().item() >= 131  # the scales really differ from block to block
        cols = list(range(k))  # every column: K <= 1536
        want = _bits(_want(w4, cols))
        for m in sorted({1, xm - 5, xm, xm + 1, 2 * xm + 3}):
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


@pytest.mark.parametrize("cfg", [0, 3])
def test_code_table_probe(cfg):
    """Every code at the ends of the scale range, in both nibble positions of every block: e = 2 and e = 127 with all
    16 codes, e = 254 with the 8 codes whose value is finite in bf16, and the three scales block by block."""
    wn, xm, st = CFGS[cfg]
    n, k = wn, STAGE * 2
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
    for m in (1, xm + 1):
        assert torch.equal(_bits(_probe(w4, cols, m, cfg, 1)), _bits(_want(w4, cols))), m


# ---- exact integer probes ------------------------------------------------------------------------------------------


class Run:
    """One config's probe points; collects every mismatch so that one run names them all."""

    def __init__(self, cfg):
        self.cfg, self.wn = cfg, CFGS[cfg][0]
        self.exact = self.bounded = 0
        self.bad = []

    def _report(self, tag, y, e, bad):
        idx = bad.nonzero()
        i, j = (int(v) for v in idx[0])
        self.bad.append(f"{tag}: {idx.shape[0]} wrong ({int(y.isnan().sum())} NaN); [{i},{j}] = {float(y[i, j]):.6g}, "
                        f"expected {float(e[i, j]):.6g}")

    def _equal(self, tag, y, e):
        self.exact += 1
        if y.shape != e.shape:
            self.bad.append(f"{tag}: shape {tuple(y.shape)} vs {tuple(e.shape)}")
        elif not torch.equal(y, e):
            self._report(tag, y, e, y.double() != e.double())

    def _close(self, tag, y, e):
        self.bounded += 1
        ok = P.close(y, e)
        if not bool(ok.all()):
            self._report(tag, y, e, ~ok)

    def point(self, mode, m, n, k, sk=1, normp=False, seed=0, p=16, frac=False):
        """mode 0 plain, 1 SwiGLU, 2 residual; every operand carved into poison (NaN; q / e bytes 0x7F = +-6 at 2^0)."""
        from chronos.ops import gemm as G

        assert G._w4m_valid(self.cfg, m, n, k, mode, sk), (self.cfg, m, n, k, mode, sk)
        tag = f"cfg {self.cfg} mode {mode}{' +norm' if normp else ''}{' frac' if frac else ''} sk {sk} M {m} N {n} K {k}"
        seed = seed * 7919 + 31 * m + 17 * n + k + mode
        x = P.carve(P.make_x(m, k, seed, DEV))
        w, q, e = W.make_w4_swiglu(n // 2, k, seed + 1, DEV) if mode == 1 else W.make_w4(n, k, seed + 1, DEV)
        q, e = P.carve(q), P.carve(e)
        part = P.carve(P.make_parts(m, k, p, seed + 2, DEV)) if normp else None
        inv = P.inv_of(part, k) if normp else None
        if mode == 2:
            r = P.carve(P.make_resid(m, n, seed + 3, DEV, frac))
            s, pt = _op(x, q, e, 2, self.cfg, sk, r)
            es, ss = P.expect_resid(x, w, r)
            self._equal(tag, s, es)
            pcols = self.wn // 2
            if pt.shape != (m, n // pcols):
                self.bad.append(f"{tag}: partials {tuple(pt.shape)}, expected {(m, n // pcols)}")
                return
            got = pt.double().sum(1)
            if frac:
                self.bounded += 1
                lim = P.part_bound(ss, pcols)
                if not bool(((got - ss).abs() <= lim).all()):
                    self.bad.append(f"{tag}: partial sums off by up to {float(((got - ss).abs() / lim).max()):.3g}x the bound")
            else:
                self.exact += 1
                if not torch.equal(got, ss):
                    self.bad.append(f"{tag}: partial sums differ in {int((got != ss).sum())} rows")
            return
        y = _op(x, q, e, mode, self.cfg, sk, None, part)[0]
        if mode == 1:
            self._close(tag, y, P.expect_swiglu(x, w, inv))
        elif normp:
            self._close(tag, y, P.expect_plain(x, w) * inv)
        else:
            self._equal(tag, y, P.expect_plain(x, w).to(torch.bfloat16))

    def thrice(self, mode, m, n, k, sk):
        """The same shape with operands A, B, A: workspace or tickets left over from one call would show in the next."""
        for seed in (1, 2, 1):
            self.point(mode, m, n, k, sk, seed=seed)

    def finish(self):
        torch.cuda.synchronize()
        print(f"\ncfg {self.cfg}: {self.exact} exact + {self.bounded} bounded comparisons")
        assert not self.bad, f"{len(self.bad)} probe points failed:\n" + "\n".join(self.bad)
        assert self.exact > 0


@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_integer_probes_stages_and_splitk(cfg):
    wn, xm, st = CFGS[cfg]
    run = Run(cfg)
    for stages in sorted({1, 2, st, st + 2}):  # stages per slice: fewer than the ring, the ring, a wrapped ring
        run.point(0, xm + 1, 3 * wn, STAGE * stages)
        run.point(2, xm + 1, wn, STAGE * stages)
        for sk in (2, 3):
            run.thrice(0, xm + 1, 3 * wn, STAGE * stages * sk, sk)
            run.thrice(2, xm + 1, wn, STAGE * stages * sk, sk)
    run.thrice(0, xm + 1, 3 * wn, STAGE * (st + 2), 1)
    run.finish()


@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_integer_probes_rows_and_epilogues(cfg):
    wn, xm, st = CFGS[cfg]
    run = Run(cfg)
    k = STAGE * (st + 2)
    for m in (1, xm, xm + 1, 2 * xm + 3):
        for n in (wn, 3 * wn):
            run.point(0, m, n, k)
            run.point(2, m, n, 2 * k, sk=2)
            run.point(1, m, n, k, normp=True)
        run.point(0, m, 3 * wn, 2 * k, sk=2, normp=True, p=6)
        run.point(1, m, 3 * wn, 3 * k, sk=3)
        run.point(2, m, 3 * wn, k, frac=True)
        run.point(2, m, wn, 3 * k, sk=3, frac=True)
    for p in (4, 72, 132):  # partial columns: fewer than a wave, more than one and two waves' lanes
        run.point(0, xm + 1, 3 * wn, k, normp=True, p=p)
        run.point(1, xm + 1, 3 * wn, k, normp=True, p=p)
    run.point(0, xm + 1, 3 * wn, 8192 + STAGE)  # K above 4096: the default group, 65 stages
    run.finish()


def test_outputs_stay_inside_their_buffers():
    """The kernel writes y, the partials and nothing around them: a launch whose outputs are the only allocations made
    between two poisoned neighbours leaves both untouched, and rows >= M of the last tile are not stored anywhere."""
    for cfg, (wn, xm, st) in CFGS.items():
        m, n, k = xm + 1, 3 * wn, STAGE * 3
        x = P.make_x(m, k, cfg, DEV)
        w, q, e = W.make_w4(n, k, cfg + 1, DEV)
        r = P.make_resid(m, n, cfg + 2, DEV)
        for sk in (1, 3):
            torch.cuda.synchronize()
            lo = P.carve(torch.zeros(4096, dtype=torch.bfloat16, device=DEV))
            s, pt = _op(x, q, e, 2, cfg, sk, r)
            hi = P.carve(torch.zeros(4096, dtype=torch.bfloat16, device=DEV))
            torch.cuda.synchronize()
            assert P.guard_ok(lo) and P.guard_ok(hi) and not bool(lo.any()) and not bool(hi.any())
            es, _ = P.expect_resid(x, w, r)
            assert torch.equal(s, es) and pt.shape == (m, n // (wn // 2))


# ---- determinism, production shapes, binding -----------------------------------------------------------------------


@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_splitk_deterministic(cfg):
    """Split-K 8 sums the slabs in slice order: five calls are bitwise equal (a replayed graph == the eager step), and
    every call leaves the tickets at zero."""
    wn, xm, st = CFGS[cfg]
    g = torch.Generator(device=DEV).manual_seed(40 + cfg)
    m, n, k = xm + 7, 4 * wn, STAGE * 8 * 3
    x = _rand((m, k), g)
    w4 = _q4(_rand((n, k), g, 0.5, 0.05))
    first, _ = _op(x, w4.q, w4.e, 0, cfg, 8)
    ref = x.float() @ w4.w.float().t()
    _check(first, ref)
    for _ in range(4):
        assert torch.equal(_op(x, w4.q, w4.e, 0, cfg, 8)[0], first)
        assert int(torch.ops.chronos.split_ticket_state(x).abs().sum()) == 0
    _check(_op(x, w4.q, w4.e, 0, cfg, 1)[0], first.float())


def _norm_parts(s, k):
    sf = s.float()
    part = torch.stack([(sf[:, i::8] ** 2).sum(1) for i in range(8)], 1).contiguous()
    return sf, part, torch.rsqrt((sf * sf).sum(1, keepdim=True) / k + 1e-5)


@pytest.mark.parametrize("m", [128, 257])
def test_8b_shapes(m):
    """One call per Llama-3-8B projection with its production epilogue (QKV plain + folded norm, O residual, gate_up
    SwiGLU + folded norm, down residual) on the cost model's pick, random data."""
    from chronos.ops import gemm as G

    g = torch.Generator(device=DEV).manual_seed(m)
    for n, k, mode, normp in ((6144, 4096, 0, True), (4096, 4096, 2, False), (28672, 4096, 1, True),
                              (4096, 14336, 2, False)):
        cfg, sk = G._w4m_model(m, n, k, mode)
        x = _rand((m, k), g, 1.0, 0.1)
        w4 = _q4(_rand((n, k), g, 0.05))
        wf = w4.w.float()
        if mode == 2:
            r = _rand((m, n), g, 4.0)
            s, part = _op(x, w4.q, w4.e, 2, cfg, sk, r)
            _check(s, (x.float() @ wf.t()).to(torch.bfloat16).float() + r.float())
            assert torch.allclose(part.sum(1), (s.float() ** 2).sum(1), rtol=1e-4, atol=1e-3)
        else:
            sf, part, inv = _norm_parts(x, k)
            hv = (sf * inv) @ wf.t()
            y = _op(x, w4.q, w4.e, mode, cfg, sk, None, part)[0]
            if mode == 1:
                _check(y, torch.nn.functional.silu(hv[:, :n // 2]) * hv[:, n // 2:], 3e-2)
            else:
                _check(y, hv)
        del w4, wf


def test_binding_checks():
    g = torch.Generator(device=DEV).manual_seed(2)
    k = STAGE * 4
    x = _rand((70, k), g)
    w4 = _q4(_rand((256, k), g))
    op = torch.ops.chronos.gemm_w4m
    y, _ = op(x, w4.q, w4.e, 0, 1, 2, None, None, 1e-5)
    _check(y, x.float() @ w4.w.float().t())
    r = _rand((70, 256), g)
    part = torch.ones(70, 8, device=DEV)

    def raises(rule, *a):
        with pytest.raises(RuntimeError, match=rule):
            op(*a)

    raises("x must be bfloat16", x.float(), w4.q, w4.e, 0, 1, 1, None, None, 1e-5)
    raises("q must be uint8", x, w4.w, w4.e, 0, 1, 1, None, None, 1e-5)                          # bf16 weights
    raises("q must be uint8", x, w4.q[:, :k // 4].contiguous(), w4.e, 0, 1, 1, None, None, 1e-5)  # q is not [N, K / 2]
    raises("e must be uint8", x, w4.q, w4.e[:, :8].contiguous(), 0, 1, 1, None, None, 1e-5)      # e is not [N, K / 32]
    raises("e must be uint8", x, w4.q, w4.e[:128].contiguous(), 0, 1, 1, None, None, 1e-5)       # ... rows
    raises("contiguous", x, w4.q.t().contiguous().t(), w4.e, 0, 1, 1, None, None, 1e-5)
    raises("contiguous", x[:, ::2], w4.q, w4.e, 0, 1, 1, None, None, 1e-5)
    raises("GPU tensor", x, w4.q.cpu(), w4.e, 0, 1, 1, None, None, 1e-5)                         # one device
    raises("gemm_w4m: cfg", x, w4.q, w4.e, 0, len(CFGS), 1, None, None, 1e-5)
    raises("gemm_w4m: cfg", x, w4.q, w4.e, 0, -1, 1, None, None, 1e-5)
    raises("gemm_w4m: mode", x, w4.q, w4.e, 3, 1, 1, None, None, 1e-5)
    raises(r"K % \(128 \* splitk\)", x, w4.q, w4.e, 0, 1, 3, None, None, 1e-5)                   # 4 stages, 3 slices
    raises(r"K % \(128 \* splitk\)", x, w4.q, w4.e, 0, 1, 0, None, None, 1e-5)
    raises("N % WN", x, w4.q[:192].contiguous(), w4.e[:192].contiguous(), 0, 1, 1, None, None, 1e-5)  # WN = 128
    raises("N % WN", x, w4.q[:192].contiguous(), w4.e[:192].contiguous(), 1, 1, 1, None, None, 1e-5)  # F = 96, WN / 2 = 64
    raises("resid mode needs resid", x, w4.q, w4.e, 2, 1, 1, None, None, 1e-5)
    raises("resid must be", x, w4.q, w4.e, 2, 1, 1, r[:69].contiguous(), None, 1e-5)
    raises("no norm prologue", x, w4.q, w4.e, 2, 1, 1, r, part, 1e-5)
    raises("part_in must be", x, w4.q, w4.e, 0, 1, 1, None, part[:69].contiguous(), 1e-5)
    raises("part_in must be", x, w4.q, w4.e, 0, 1, 1, None, part.double(), 1e-5)
    s, pt = op(x, w4.q, w4.e, 2, 1, 1, r, None, 1e-5)  # and the accepted residual call next to them
    _check(s, (x.float() @ w4.w.float().t()).to(torch.bfloat16).float() + r.float())
    assert pt.shape == (70, 256 // 64)


# ---- routing -------------------------------------------------------------------------------------------------------


def _wx(m, n, k, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(m, k, device=DEV, generator=g) + 0.1).to(torch.bfloat16)
    return x, _q4((torch.randn(n, k, device=DEV, generator=g) * 0.02).to(torch.bfloat16)), g


def test_routing_switch(switch):
    from chronos import ops
    from chronos.ops import gemm
    from chronos.ops.gemm import LazyNorm

    m, n, k = 80, 512, 1024  # no "w4mplans" row
    x, w4, g = _wx(m, n, k, 2)
    wf = w4.w.float()
    xr = (torch.randn(m, n, device=DEV, generator=g) + 0.1).to(torch.bfloat16)
    wd = _q4((torch.randn(k, n, device=DEV, generator=g) * 0.02).to(torch.bfloat16))  # [N = 1024, K = 512]
    sf, part, inv = _norm_parts(x, k)
    lazy = lambda: LazyNorm(x, part, torch.ones(k, device=DEV, dtype=torch.bfloat16), 1e-5)  # noqa: E731
    count = lambda: gemm.w4_stats["mid_launches"]  # noqa: E731
    resid = torch.randn(m, k, device=DEV, generator=g).to(torch.bfloat16)

    for mode in ("plan", "off"):
        switch(mode)
        c0 = count()
        assert gemm.w4m_plan(m, n, k) is None and gemm.w4m_plan(m, n, k, 0, True) is None
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
    out = ops.gemv_resid(xr, wd, resid)
    assert count() == c0 + 5 and out.part.shape[0] == m and out.s.shape == resid.shape
    _check(out.s, (xr.float() @ wd.w.float().t()).to(torch.bfloat16).float() + resid.float())
    assert torch.allclose(out.part.sum(1), (out.s.float() ** 2).sum(1), rtol=1e-4, atol=1e-3)
    buf = torch.empty(m, n, device=DEV, dtype=torch.bfloat16)
    assert torch.equal(ops.linear(x, w4, out=buf), ops.linear(x, w4.w)) and count() == c0 + 5  # out= is not routed
    assert torch.equal(ops.linear(x[:64], w4), ops.linear(x[:64], w4.w)) and count() == c0 + 5  # M = 64: not this kernel
    gemm._W4A16_DECODE = False  # CHRONOS_W4A16_DECODE=0 still forces the copy everywhere
    try:
        assert torch.equal(ops.linear(x, w4), ops.linear(x, w4.w))
        assert count() == c0 + 5
    finally:
        gemm._W4A16_DECODE = True
    switch("off")
    assert torch.equal(ops.linear(x, w4), ops.linear(x, w4.w)) and count() == c0 + 5


def test_beats_one_rows_route_packed_tensors_only(switch, monkeypatch, tmp_path):
    from chronos import ops
    from chronos.models.llama import Q4Tensor
    from chronos.ops import gemm

    m, n, k = 100, 512, 1024
    x, w4, g = _wx(m, n, k, 6)
    wp = Q4Tensor(w4.q, w4.e, None)  # the packed-only form of the same weight
    wp.scratch = ops.W4Scratch(n * k, DEV)
    path = tmp_path / "plan.json"
    path.write_text(json.dumps({"w4mplans": {f"{n},{k},0": [[128, 0, 2, 1]], f"{n},{k},1": [[128, 0, 1, 2]]}}))
    monkeypatch.setenv("CHRONOS_GEMM_PLAN", str(path))
    reset = gemm._reset_plans
    reset()
    try:
        switch("plan")
        c0 = dict(gemm.w4_stats)
        copy = ops.linear(x, w4)                      # beats 1: the copy-mode tensor keeps its bf16 kernel
        assert gemm.w4_stats == c0 and torch.equal(copy, ops.linear(x, w4.w))
        y = ops.linear(x, wp)                         # ... and the packed tensor takes the kernel: no expansion
        assert gemm.w4_stats["mid_launches"] == c0["mid_launches"] + 1
        assert gemm.w4_stats["expand_launches"] == c0["expand_launches"]
        _check(y, x.float() @ w4.w.float().t())
        assert torch.equal(y, _op(x, w4.q, w4.e, 0, 0, 2)[0])
        ops.gate_up_silu(x, w4)                       # beats 2: both
        ops.gate_up_silu(x, wp)
        assert gemm.w4_stats["mid_launches"] == c0["mid_launches"] + 3
        assert gemm.w4_stats["expand_launches"] == c0["expand_launches"]
        assert torch.equal(ops.linear(x[:70].repeat(3, 1), wp), ops.linear(x[:70].repeat(3, 1), w4.w))  # M = 210: no row
        assert gemm.w4_stats["expand_launches"] == c0["expand_launches"] + 1
    finally:
        monkeypatch.delenv("CHRONOS_GEMM_PLAN")
        reset()


# ---- model and engine ----------------------------------------------------------------------------------------------


def _it(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _prefill244(m):
    """A 4 x 61-token prefill (M = 244): (logits, launch counts)."""
    from chronos.models.llama import KVCache, make_prefill_batch
    from chronos.ops import gemm

    prompts = [list(range(100 + 7 * b, 161 + 7 * b)) for b in range(4)]
    bts = [list(range(1 + 5 * b, 6 + 5 * b)) for b in range(4)]
    kv = KVCache(m.cfg, m.tp, 32, 16, DEV)
    kv.buf.zero_()
    c0 = dict(gemm.w4_stats)
    out = m.forward(make_prefill_batch(prompts, [0] * 4, bts, m.cfg, m.tp, DEV, max_blocks=8, nqt=8), kv)
    return out.float(), {k: v - c0[k] for k, v in gemm.w4_stats.items()}


def _decode80(m):
    """An 80-row decode step over a seeded KV cache: (logits, launch counts)."""
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
    c0 = dict(gemm.w4_stats)
    out = m.forward(sb, kv)
    return out.float(), {k: v - c0[k] for k, v in gemm.w4_stats.items()}


@pytest.mark.parametrize("weights", ["mxfp4-packed", "mxfp4"])
def test_mxfp4_model_mid_vs_bf16_route(switch, weights):
    """"small" under W4_MID = "model": the M = 244 prefill and an 80-row decode step run all four projections of every
    layer on the kernel (K = 1024 and the down projection's K = 2816 = 22 x 128 alike) — in packed-only mode without a
    single expansion — and give the logits of the bf16 route within the project's bound for this comparison."""
    from chronos.models.llama import build_model

    m = build_model("small", DEV, seed=5, weight_dtype=weights)
    assert m.w.w4 and (m.w.layers[0].wqkv.w is None) == (weights == "mxfp4-packed")
    L = m.cfg.num_layers
    res = {}
    for name in ("model", "off"):
        switch(name)
        res[name] = (_prefill244(m), _decode80(m))
    cos = lambda a, b: torch.nn.functional.cosine_similarity(a, b, dim=-1).min().item()  # noqa: E731
    for i, what in enumerate(("prefill 244", "decode 80")):
        (ym, nm), (yo, no) = res["model"][i], res["off"][i]
        print(what, weights, "min cosine", cos(ym, yo), nm, no)
        assert nm["mid_launches"] == 4 * L and nm["expand_launches"] == 0, (what, nm)
        assert no["mid_launches"] == 0 and no["expand_launches"] == (4 * L if weights == "mxfp4-packed" else 0), (what, no)
        assert cos(ym, yo) > 0.995, what


@pytest.mark.parametrize("weights", ["mxfp4", "mxfp4-packed"])
def test_mxfp4_engine_mid(switch, weights):
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
        eng = Engine(EngineConfig(model="small", device="cuda:0", max_slots=96, max_model_len=256, decode_burst=4,
                                  weight_dtype=weights))
        assert eng.cfg.use_graphs and eng.model.w.w4
        before = gemm.w4_stats["mid_launches"]
        reqs = [eng.submit(build_prompt(c), fmt=VERDICT_SCHEMA, num_predict=40) for c in chains]
        eng.run_until_idle()
        torch.cuda.synchronize()
        for r in reqs:
            assert r.error is None
            assert {"risk_score", "verdict", "reason"} <= set(json.loads(r.text)), r.text
        assert gemm.w4_stats["mid_launches"] > before
        texts.append([r.text for r in reqs])
        del eng
    assert texts[0] == texts[1]  # graph replay and the split-K order are stable
