"""Exact integer probes (tests/_gemm_probes.py) through every hand-written projection GEMM config and epilogue.

One test per config of ``gemm_pp`` (gemm_pp.hip 0-11, gemm_lg.hip 12-39 / 72-80, the HB slab loop 81-94), of
``gemm_skinny`` (bf16 configs 0-11) and of the fp8 ``qgemm_lg`` (0-4), plus the decode GEMV family and the older MFMA
``gemm``.  tests/test_gemm_probes.py (CPU) proves the builders, shows which mutations the probes notice, and fails when
the lists below stop being the op's tables (``test_gpu_lists_are_the_ops_tables``).

What is swept per tile config (all shapes small: M <= 515 but for one nine-tile point, N <= 520, K <= 2496):
* stages: split-K 1 at every K = 64 kts that gives 1 .. ST + 2 ring stages (ST, and the LDS row bytes that say how many
  stages one 64-k unit is, are read from the config table in csrc/kernels/gemm_lg.hip; gemm_pp 0-11 and the HB
  configs, whose loop is unrolled by two slabs: kts = 1 .. 5) — plain at M = XM + 1, N = WN + 4, residual at N = WN;
* split-K 2 and 3 with 1, 2 and ST + 1 stages per slice, then the same shape with other operands, then the first
  again: stale workspace or tickets would show;
* rows M in {1, XM - 1, XM, XM + 1, 2 XM + 3} and, plain, columns N in {4, WN - 4, WN + 4, 2 WN + 8};
* every epilogue (plain, plain + folded norm, SwiGLU with and without it, residual + RMSNorm partials, the residual
  with a fractional r) at N = 2 WN with and without split-K; the norm prologue also with 4, 6, 72 and 132 partial
  columns, and one plain point with nine x tiles (more than one group of the grouped tile order).
On top of the per-config sweeps, every (config, split-K, K, epilogue) that ops/gemm_plan.json routes runs at its
production K (``test_routed_row_at_production_k``), and a negative control shows a mutated operand through the kernels.
Every (config, mode, split-K, M, N, K) is asked of ``ops.gemm._pp_valid`` / ``_sk_valid`` first; what the op rejects is
left out (and listed by ``-s``), and every config must keep plain mode and at least one fused mode.

Plain and residual outputs are compared with ``torch.equal``, the residual's partials after an fp64 column sum by
equality; SwiGLU and the norm prologue within 2^-7 of the fp64 expectation (the derivation is in _gemm_probes.py).
Nothing here is relative to max|ref|.
"""
import os
import re

import pytest
import torch

import _gemm_probes as P

DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PP = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]  # gemm_pp.hip
LG = [12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39,
      72, 73, 74, 75, 76, 77, 78, 79, 80]  # gemm_lg.hip ring / slab schedules
HB = [81, 82, 83, 84, 85, 86, 87, 88, 89, 90, 91, 92, 93, 94]  # gemm_lg.hip HB slab loop
SK = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]  # gemm_skinny.hip, bf16 weights
F8 = [0, 1, 2, 3, 4]  # gemm_lg.hip fp8 configs (qgemm_lg)


def _table(macro):
    """{id: (WN, XM, RB, ST)} of a config X-macro in csrc/kernels/gemm_lg.hip."""
    with open(os.path.join(REPO, "csrc", "kernels", "gemm_lg.hip")) as fh:
        src = fh.read()
    body = re.search(r"#define " + macro + r"\(X\)((?:.*\\\n)*.*\n)", src).group(1)
    rows = re.findall(r"X\((\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),", body)
    return {int(r[0]): tuple(int(v) for v in r[1:5]) for r in rows}


LG_GEO = _table("LG_CONFIGS")
F8_GEO = _table("LG_F8_CONFIGS")
CASES = [pytest.param(("pp", c), id=f"pp{c}") for c in PP + LG + HB] + \
        [pytest.param(("sk", c), id=f"skinny{c}") for c in SK] + [pytest.param(("f8", c), id=f"fp8_{c}") for c in F8]


def splitk_ok(cfg):
    return not (HB[0] <= cfg <= HB[-1]) or cfg >= 88  # gemm_lg_splitk_ok; gemm_pp 0-11 all have the path


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from chronos import ops

    ops.load()
    import chronos.native as n

    assert "_C" in n._loaded


class Run:
    """One config's probe points: launches, compares, and collects every mismatch so one run names them all."""

    def __init__(self, name, launch, valid, pcols):
        self.name, self.launch, self.valid, self.pcols = name, launch, valid, pcols
        self.exact = self.bounded = 0
        self.rejected, self.bad, self.modes = set(), [], set()

    def _call(self, *args):
        try:
            out = self.launch(*args)
            torch.cuda.synchronize()
            return out
        except RuntimeError as exc:
            if "chronos:" in str(exc):  # a binding check: the op rejects what its _valid function accepts
                self.bad.append(f"rejected by the binding: {str(exc).splitlines()[0]}")
                return None
            pytest.exit(f"device error in {self.name}: {exc}", returncode=3)  # nothing after a fault can be trusted

    def _cmp_equal(self, tag, y, e):
        if y is None:  # (the rejection is already recorded)
            return
        self.exact += 1
        if y.shape != e.shape or not torch.equal(y, e):
            self._report(tag, y, e, y.double() != e.double() if y.shape == e.shape else None)

    def _cmp_close(self, tag, y, e):
        if y is None:
            return
        self.bounded += 1
        ok = P.close(y, e)
        if not bool(ok.all()):
            self._report(tag, y, e, ~ok)

    def _report(self, tag, y, e, bad):
        if bad is None:
            self.bad.append(f"{tag}: shape {tuple(y.shape)} vs {tuple(e.shape)}")
            return
        idx = bad.nonzero()
        i, j = (int(v) for v in idx[0])
        rows, cols = idx[:, 0].unique(), idx[:, 1].unique()
        self.bad.append(f"{tag}: {idx.shape[0]} wrong ({int(y.isnan().sum())} NaN) in rows {int(rows.min())}-"
                        f"{int(rows.max())} ({rows.numel()}), cols {int(cols.min())}-{int(cols.max())} ({cols.numel()});"
                        f" [{i},{j}] = {float(y[i, j]):.6g}, expected {float(e[i, j]):.6g}")

    def point(self, mode, m, n, k, sk=1, normp=False, seed=0, p=16, frac=False):
        """mode 0 plain, 1 SwiGLU, 2 residual.  False when the op rejects the combination."""
        if not self.valid(m, n, k, mode, sk):
            self.rejected.add((("plain", "swiglu", "resid")[mode], f"sk{sk}" if sk > 1 else "", f"N{n}", f"K{k}"))
            return False
        self.modes.add((mode, normp))
        tag = f"{self.name} mode {mode}{' +norm' if normp else ''}{' frac' if frac else ''} sk {sk} M {m} N {n} K {k}"
        seed = seed * 7919 + 31 * m + 17 * n + k + mode
        x = P.carve(P.make_x(m, k, seed, DEV))
        w = P.carve(P.make_w_swiglu(n // 2, k, seed + 1, DEV) if mode == 1 else P.make_w(n, k, seed + 1, DEV))
        part = P.carve(P.make_parts(m, k, p, seed + 2, DEV)) if normp else None
        inv = P.inv_of(part, k) if normp else None
        if mode == 2:
            r = P.carve(P.make_resid(m, n, seed + 3, DEV, frac))
            out = self._call(x, w, mode, sk, r, None)
            if out is None:
                return True
            s, ss = P.expect_resid(x, w, r)
            self._cmp_equal(tag, out[0], s)
            got = out[1].double().sum(1)
            if out[1].shape != (m, n // self.pcols):
                self.bad.append(f"{tag}: partials {tuple(out[1].shape)}, expected {(m, n // self.pcols)}")
            elif frac:
                self.bounded += 1
                lim = P.part_bound(ss, self.pcols)
                if not bool(((got - ss).abs() <= lim).all()):
                    self.bad.append(f"{tag}: partial sums off by up to {float(((got - ss).abs() / lim).max()):.3g}x the bound")
            else:
                self.exact += 1
                if not torch.equal(got, ss):
                    rows = (got != ss).nonzero().flatten()
                    self.bad.append(f"{tag}: partial sums differ in {rows.numel()} rows, first {int(rows[0])}: "
                                    f"{float(got[rows[0]])} vs {float(ss[rows[0]])}")
            return True
        out = self._call(x, w, mode, sk, None, part)
        if out is None:
            return True
        y = out[0]
        if mode == 1:
            self._cmp_close(tag, y, P.expect_swiglu(x, w, inv))
        elif normp:
            self._cmp_close(tag, y, P.expect_plain(x, w) * inv)
        else:
            self._cmp_equal(tag, y, P.expect_plain(x, w).to(torch.bfloat16))
        return True

    def thrice(self, mode, m, n, k, sk):
        """The same shape with operands A, B, A: workspace or tickets left over from one call would show in the next."""
        for seed in (1, 2, 1):
            self.point(mode, m, n, k, sk, seed=seed)

    def finish(self, every_mode=True):
        print(f"\n{self.name}: {self.exact} exact + {self.bounded} bounded comparisons; rejected by the op: "
              f"{sorted(self.rejected) or 'none'}")
        assert not self.bad, f"{len(self.bad)} probe points failed:\n" + "\n".join(self.bad)
        if every_mode:
            assert (0, False) in self.modes, "plain mode never ran"
            assert any(md != (0, False) for md in self.modes), "no fused mode ran"
        assert self.exact > 0


def _ceil(a, b):
    return -(-a // b)


def _pp_runner(cfg):
    from chronos.ops import gemm as G

    if cfg in LG_GEO:
        wn, xm, rb, st = LG_GEO[cfg]
        spk = 128 // rb  # ring stages per 64-k unit
    else:
        wn, xm, st, spk = G._PP_BN[cfg], G._PP_BM[cfg], 2, 1
    assert (wn, xm) == (G._PP_BN[cfg], G._PP_BM[cfg])

    def launch(x, w, mode, sk, resid, part):
        return torch.ops.chronos.gemm_pp(x, w, mode, cfg, sk, resid, part, P.EPS, False)

    run = Run(f"gemm_pp cfg {cfg}", launch, lambda m, n, k, mode, sk: G._pp_valid(cfg, n, k, mode, sk, m),
              wn // 2 if cfg >= G.LG_FIRST else wn // 4)
    return run, wn, xm, st, spk


def _sk_runner(cfg):
    from chronos.ops import gemm as G

    rt, mt, nw = G._SK[cfg]

    def launch(x, w, mode, sk, resid, part):
        return torch.ops.chronos.gemm_skinny(x, w, mode, cfg, sk, resid, part, P.EPS)

    run = Run(f"gemm_skinny cfg {cfg}", launch, lambda m, n, k, mode, sk: G._sk_valid(cfg, m, n, k, mode, sk), 16 * rt)
    return run, rt, mt, nw


def _run_pp(cfg):
    run, wn, xm, st, spk = _pp_runner(cfg)
    # gemm_pp 0-11 and the HB loop (unrolled by two slabs: both parities and the one-slab case): kts = 1 .. 5
    kts_sweep = range(1, 6) if cfg in HB or cfg in PP else range(1, (st + 2) // spk + 1)
    m1 = xm + 1
    for kts in kts_sweep:  # the prologue / drain at every stage count around the ring depth
        run.point(0, m1, wn + 4, 64 * kts)
        run.point(2, m1, wn, 64 * kts)
    kslice = sorted({_ceil(s, spk) for s in (1, 2, st + 1)})
    sks = [2, 3] if splitk_ok(cfg) else []
    for sk in sks:
        for kts in kslice:
            run.thrice(0, m1, wn + 4, 64 * kts * sk, sk)
    for sk in (2, 3):
        if sk not in sks:
            assert not run.point(0, m1, wn + 4, 64 * sk, sk)  # (recorded as rejected)
    kd = 64 * _ceil(st + 1, spk)  # ST + 1 stages: one more than the ring holds
    for m in (1, xm - 1, xm, xm + 1, 2 * xm + 3):
        run.point(0, m, wn + 4, kd)
    for n in (4, wn - 4, wn + 4, 2 * wn + 8):
        run.point(0, m1, n, kd)
    for sk in [1] + sks[:1]:
        for mode, normp, frac in ((0, False, False), (0, True, False), (1, False, False), (1, True, False),
                                  (2, False, False), (2, False, True)):
            run.point(mode, m1, 2 * wn, kd * sk, sk, normp, frac=frac)
    run.point(0, m1, 2 * wn, kd, 1, True, p=72)  # more partials than a wave has lanes
    run.point(1, 2 * xm + 3, 2 * wn, kd, 1, True, p=4)
    run.point(0, m1, 2 * wn, kd, 1, True, p=6)  # P % 4 != 0: gemm_lg's scalar read of the partials
    run.point(1, m1, 2 * wn, kd, 1, True, p=132)  # two more rounds of 64 after the first
    # nine x tiles: more than one group of the grouped tile order (knob pp_gm = 8), the last group of one
    run.point(0, 8 * xm + 1, 2 * wn + 4, kd)
    run.finish()


def _run_skinny(cfg):
    run, rt, mt, nw = _sk_runner(cfg)
    n = 16 * rt * 3
    ms = sorted({1, 2, 16 * mt - 1, 16 * mt})
    for sk in (1, 2, 3):
        for u in (1, 2, 3):  # 64-k units per wave: one is the whole loop in its prologue
            k = 64 * nw * sk * u
            for m in ms:
                for mode, normp, frac in ((0, False, False), (0, True, False), (1, False, False), (1, True, False),
                                          (2, False, False), (2, False, True)):
                    run.point(mode, m, n, k, sk, normp, p=8, frac=frac)
            m = 16 * mt - 1
            if sk > 1:
                run.thrice(0, m, n, k, sk)
                run.thrice(2, m, n, k, sk)
    run.point(0, 16 * mt, n, 64 * nw * 2, 1, True, p=72)
    run.point(0, 1, n, 64 * nw * 2, 2, True, p=4)
    run.point(0, 16 * mt - 1, n, 64 * nw * 2, 1, True, p=6)
    run.point(0, 16 * mt - 1, n, 64 * nw * 2, 1, True, p=132)  # two more rounds of 64 after the first
    run.finish()


def _run_f8(cfg):
    from chronos.ops import gemm as G

    wn, xm, rb, st = F8_GEO[cfg]
    assert G.QLG_GEO[cfg] == (xm, wn)
    run = Run(f"qgemm_lg cfg {cfg}", None, None, 0)

    def point(swiglu, m, n, k, sk=1, seed=0):
        # the binding's own rules (bindings.cpp qgemm_lg)
        if k % 128 or (k // 128) % sk or (n % wn if swiglu else n % 4):
            run.rejected.add(("swiglu" if swiglu else "plain", f"sk{sk}", f"N{n}", f"K{k}"))
            return
        run.modes.add((int(swiglu), False))
        tag = f"{run.name} {'swiglu' if swiglu else 'plain'} sk {sk} M {m} N {n} K {k}"
        seed = seed * 7919 + 31 * m + 17 * n + k + swiglu
        x = P.make_x(m, k, seed, DEV)
        w = P.make_w_swiglu(n // 2, k, seed + 1, DEV) if swiglu else P.make_w(n, k, seed + 1, DEV)
        xs, ws = P.carve(P.pow2_scales(m, DEV)), P.carve(P.pow2_scales(n, DEV))
        xq, wq = P.carve(P.to_e4m3(x)), P.carve(P.to_e4m3(w))
        run.launch = lambda *a: torch.ops.chronos.qgemm_lg(xq, xs, wq, ws, swiglu, cfg, sk)
        y = run._call()
        if y is None:
            return
        h = P.expect_plain(x, w) * xs.double()[:, None] * ws.double()[None, :]
        if swiglu:
            g, u = h[:, :n // 2], h[:, n // 2:]
            run._cmp_close(tag, y, g / (1.0 + torch.exp(-g)) * u)
        else:
            run._cmp_equal(tag, y, h.to(torch.bfloat16))

    m1 = xm + 1
    for units in range(1, (6 if cfg == 4 else st + 3)):  # one k-unit = one 128-deep stage
        point(False, m1, wn + 4, 128 * units)
        point(True, m1, 2 * wn, 128 * units)
    kd = 128 * (st + 1)
    for m in (1, xm - 1, xm, xm + 1, 2 * xm + 3):
        point(False, m, wn + 4, kd)
    for n in (4, wn - 4, wn + 4, 2 * wn + 8):
        point(False, m1, n, kd)
    for u in (1, 2, st + 1):
        for seed in (1, 2, 1):
            point(False, m1, wn + 4, 128 * 2 * u, 2, seed)
        point(True, m1, 2 * wn, 128 * 2 * u, 2)
    point(True, 2 * xm + 3, wn, kd)
    run.finish()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_config(case):
    fam, cfg = case
    {"pp": _run_pp, "sk": _run_skinny, "f8": _run_f8}[fam](cfg)


@pytest.mark.gpu
def test_configs_without_a_splitk_path_are_rejected_not_run():
    x = torch.zeros(256, 128, dtype=torch.bfloat16, device=DEV)
    for cfg in HB:
        if not splitk_ok(cfg):
            with pytest.raises(RuntimeError, match="split-K"):
                torch.ops.chronos.gemm_pp(x, x, 0, cfg, 2, None, None, 1e-5, False)


@pytest.mark.gpu
@pytest.mark.parametrize("handoff", [0, 1], ids=["fences", "write_through"])
def test_lg_splitk_handoff_forms(handoff):
    """gemm_lg's split-K slab hand-off has two forms (plain stores + agent fences, write-through stores + agent-scope
    loads); the default picks by tile size, so each config above ran only one.  Knob lg_handoff forces the other."""
    torch.ops.chronos.set_knob("lg_handoff", handoff)
    try:
        for cfg in LG:
            run, wn, xm, st, spk = _pp_runner(cfg)
            run.name += f" lg_handoff {handoff}"
            for sk in (2, 3):
                run.thrice(0, xm + 1, wn + 4, 64 * sk * _ceil(st + 1, spk), sk)
            run.point(2, xm + 1, wn, 64 * 2, 2)
            run.point(1, xm + 1, 2 * wn, 64 * 4, 2, True)
            run.finish()
    finally:
        torch.ops.chronos.set_knob("lg_handoff", -1)


# ---- the routed plan rows at their production K -------------------------------------------------------------------
def _routed():
    """Every (config, split-K, K, epilogue) ops/gemm_plan.json routes to a hand-written bf16 kernel / fp8 config."""
    import json

    with open(os.path.join(REPO, "project-chronos-distributed-behavioral-edr-ebpf-llm-_amd", "ops", "gemm_plan.json")) as fh:
        plan = json.load(fh)
    bf, f8 = set(), set()
    for key, rows in plan["plans"].items():
        _, k, mode = (int(v) for v in key.split(","))
        bf |= {(r[1], r[2], k, mode) for r in rows if r[1] >= 0}
    for key, rows in plan.get("qplans", {}).items():
        _, k, sw = (int(v) for v in key.split(","))
        f8 |= {(r[1] - 10, r[2] if len(r) > 2 else 1, k, sw) for r in rows if r[1] >= 10}
    return sorted(bf), sorted(f8)


ROUTED, ROUTED_F8 = _routed()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROUTED, ids=lambda r: "cfg{}-sk{}-K{}-mode{}".format(*r))
def test_routed_row_at_production_k(row):
    """The production K and split-K of every routed row (K = 4096 split 8 is 8 units on a ring 8 deep; K = 28672 is 64
    non-zeros per W row over 448-row groups), on a two-tile N and a ragged M: what test_gemm_plan_gpu.py checks to
    1e-2 max|ref| + 2^-7 |ref| at the full N, exactly."""
    cfg, sk, k, mode = row
    if cfg >= 100:
        run, rt, mt, _ = _sk_runner(cfg - 100)
        m, n = 16 * mt - 1, 16 * rt * 4
    else:
        run, wn, xm, _, _ = _pp_runner(cfg)
        m, n = xm + 1, 2 * wn
    assert run.point(mode, m, n, k, sk)
    if mode == 2:
        run.point(mode, m, n, k, sk, frac=True)
    else:
        run.point(mode, m, n, k, sk, True)  # the decoder calls these with the folded norm
        run.point(0, m, n, k, sk)
    if sk > 1:
        run.thrice(0, m, n, k, sk)
    run.finish(every_mode=False)


@pytest.mark.gpu
def test_routed_fp8_rows_at_production_k():
    assert ROUTED_F8
    for cfg, sk, k, sw in ROUTED_F8:
        wn, xm, _, _ = F8_GEO[cfg]
        run = Run(f"qgemm_lg cfg {cfg}", None, None, 0)
        m, n = xm + 1, 2 * wn
        x, w = P.make_x(m, k, k + cfg, DEV), P.make_w(n, k, k + cfg + 1, DEV)
        xs, ws = P.carve(P.pow2_scales(m, DEV)), P.carve(P.pow2_scales(n, DEV))
        xq, wq = P.carve(P.to_e4m3(x)), P.carve(P.to_e4m3(w))
        run.launch = lambda: torch.ops.chronos.qgemm_lg(xq, xs, wq, ws, False, cfg, sk)
        e = P.expect_plain(x, w) * xs.double()[:, None] * ws.double()[None, :]
        run._cmp_equal(f"{run.name} sk {sk} K {k}", run._call(), e.to(torch.bfloat16))
        run.finish(every_mode=False)


@pytest.mark.gpu
def test_a_mutated_operand_is_seen_through_the_kernels():
    """Negative control: the kernels run on an x with one k column zeroed while the expectation keeps it.  Every
    output column whose W row holds that k must then differ from the expectation by >= 1 somewhere in each 16 rows —
    the comparison is not vacuous, on the device, through the real launch path."""
    m, n, k, k0 = 32, 128, 1024, 515
    x, w = P.make_x(m, k, 1, DEV), P.make_w(n, k, 2, DEV)
    e = P.expect_plain(x, w)
    xz = x.clone()
    xz[:, k0] = 0
    cols = w[:, k0] != 0
    assert int(cols.sum()) == n // P.group(k)
    ops = torch.ops.chronos
    outs = {"gemm_pp 3": ops.gemm_pp(xz, w, 0, 3, 1, None, None, 1e-5, False)[0],
            "gemm_lg 19": ops.gemm_pp(xz, w, 0, 19, 2, None, None, 1e-5, False)[0],
            "hb 88": ops.gemm_pp(xz, w, 0, 88, 1, None, None, 1e-5, False)[0],
            "skinny 6": ops.gemm_skinny(xz, w, 0, 6, 2, None, None, 1e-5)[0],
            "gemm": ops.gemm(xz, w, False, 3), "gemv": ops.gemv(xz[:8], w, False)}
    for name, y in outs.items():
        rows = y.shape[0]
        d = (y.double() - e[:rows]).abs()
        assert torch.equal(d[:, ~cols], torch.zeros_like(d[:, ~cols])), name
        hit = (d >= 1).view(-1, min(rows, 16), n).any(1)
        assert bool(hit[:, cols].all()), name


# ---- the decode GEMV family (gemv.hip, bf16 weights) --------------------------------------------------------------
@pytest.fixture(params=[0, 37], ids=["grid", "persist37"])
def persist(request):
    """gemv.hip knob gemv_persist: 0 = one workgroup per row group, 37 = a 37-workgroup grid looping over the groups."""
    torch.ops.chronos.set_knob("gemv_persist", request.param)
    yield request.param
    torch.ops.chronos.set_knob("gemv_persist", -1)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [512, 1024, 1536])
def test_gemv(k, persist):
    """``gemv`` (plain, SwiGLU) at M in {1, 2, 3, 8}, ``gemv_resid`` and ``gemv_normp`` at M in {1, 2}; N = 16 is one
    row group, 48 an odd number of them, 4096 + 16 more groups than the persistent grid has workgroups.

    The folded norm multiplies the fp32 row sums by inv before the bf16 rounding (gemv.hip: ``totw`` times ``invm``),
    it does not round s inv first — the rounding tests/test_decode_fusion_gpu.py speaks of is the unfused chain's — so
    the module's 2^-7 bound holds here without an extra term."""
    ops = torch.ops.chronos
    run = Run(f"gemv K {k} persist {persist}", None, lambda *a: True, 0)

    def call(fn):
        run.launch = fn
        return run._call()

    for n in (16, 48, 4096 + 16):
        for m in (1, 2, 3, 8):
            seed = 100 * m + n + k
            x = P.carve(P.make_x(m, k, seed, DEV))
            w = P.carve(P.make_w(n, k, seed + 1, DEV))
            wg = P.carve(P.make_w_swiglu(n // 2, k, seed + 2, DEV))
            tag = f"{run.name} M {m} N {n}"
            run.modes.add((0, False))
            run._cmp_equal(tag + " gemv", call(lambda: ops.gemv(x, w, False)), P.expect_plain(x, w).to(torch.bfloat16))
            run.modes.add((1, False))
            run._cmp_close(tag + " gemv swiglu", call(lambda: ops.gemv(x, wg, True)), P.expect_swiglu(x, wg))
            if m > 2:
                continue
            for frac in (False, True):
                r = P.carve(P.make_resid(m, n, seed + 3, DEV, frac))
                out = P.carve(torch.zeros(m, n, dtype=torch.bfloat16, device=DEV))
                part = call(lambda: ops.gemv_resid(x, w, r, out))
                s, ss = P.expect_resid(x, w, r)
                run._cmp_equal(tag + f" gemv_resid frac {frac}", out, s)
                if not P.guard_ok(out):
                    run.bad.append(tag + " gemv_resid wrote outside resid_out")
                got = part.double().sum(1)
                # at most 8 rows per workgroup: a partial is a sum of <= 8 squares
                ok = ((got - ss).abs() <= P.part_bound(ss, 8)).all() if frac else torch.equal(got, ss)
                if not bool(ok):
                    run.bad.append(tag + f" gemv_resid frac {frac}: partial sums {got.tolist()} vs {ss.tolist()}")
            npart = k // (4 if m == 1 else 8)  # what gemv_resid emits for a K-wide residual stream
            pin = P.carve(P.make_parts(m, k, npart, seed + 4, DEV))
            inv = P.inv_of(pin, k)
            run._cmp_close(tag + " gemv_normp", call(lambda: ops.gemv_normp(x, pin, P.EPS, w, False)),
                           P.expect_plain(x, w) * inv)
            run._cmp_close(tag + " gemv_normp swiglu", call(lambda: ops.gemv_normp(x, pin, P.EPS, wg, True)),
                           P.expect_swiglu(x, wg, inv))
    run.finish()


# ---- the older MFMA GEMM (gemm.hip) -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stages", [2, 3])
def test_mfma_gemm(stages):
    run = Run(f"gemm stages {stages}", None, lambda *a: True, 0)
    for m in (3, 129):
        for k in (64, 128, 640):  # 1, 2 and 10 64-deep steps: fewer than, as many as and more than the ring holds
            for n in (128, 384):
                seed = m + k + n
                x = P.carve(P.make_x(m, k, seed, DEV))
                w = P.carve(P.make_w(n, k, seed + 1, DEV))
                wg = P.carve(P.make_w_swiglu(n // 2, k, seed + 2, DEV))
                tag = f"{run.name} M {m} N {n} K {k}"
                run.launch = lambda: torch.ops.chronos.gemm(x, w, False, stages)
                run.modes.add((0, False))
                run._cmp_equal(tag, run._call(), P.expect_plain(x, w).to(torch.bfloat16))
                run.launch = lambda: torch.ops.chronos.gemm(x, wg, True, stages)
                run.modes.add((1, False))
                run._cmp_close(tag + " swiglu", run._call(), P.expect_swiglu(x, wg))
    run.finish()
