"""Routing of the W8A16 skinny GEMM (ops/gemm.py w8_plan): the "w8plans" section of gemm_plan.json, the validity
predicate against the binding's rules, the committed rows, the CPU path, what default and ``a16`` calls launch on an fp8
weight (through the tests/_gemm_dispatch.py recorder) and the engine's config field."""
import itertools
import json
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "profiles", "fp8", "skinny_table.jsonl")
SHAPES_8B = ((6144, 4096, 0), (4096, 4096, 2), (28672, 4096, 1), (4096, 14336, 2))
SMALL = ((1536, 1024, 0), (1024, 1024, 2), (5632, 1024, 1), (1024, 2816, 2))


@pytest.fixture
def gemm():
    """ops/gemm.py with its plan tables, cache and switch restored afterwards."""
    from chronos.ops import gemm as g

    old = g.W8_SKINNY
    try:
        yield g
    finally:
        g.W8_SKINNY = old
        g._reset_plans()


def _load(gemm, monkeypatch, tmp_path, raw):
    path = tmp_path / "plan.json"
    path.write_text(json.dumps(raw))
    monkeypatch.setenv("CHRONOS_GEMM_PLAN", str(path))
    gemm._reset_plans()


def test_w8plans_section_parses(gemm, monkeypatch, tmp_path):
    gemm.W8_SKINNY = "plan"
    _load(gemm, monkeypatch, tmp_path, {"plans": {}, "w8plans": {"6144,4096,0": [[2, -1, 1], [5, 0, 1], [16, 2, 2],
                                                                                  [64, -1, 1]]}})
    assert gemm.w8_plan(2, 6144, 4096, 0) is None          # cfg < 0: measured and lost
    assert gemm.w8_plan(3, 6144, 4096, 0) == (0, 1)        # (2, 5]
    assert gemm.w8_plan(5, 6144, 4096, 0) == (0, 1)
    assert gemm.w8_plan(8, 6144, 4096, 0) == (2, 2)        # (5, 16]
    assert gemm.w8_plan(17, 6144, 4096, 0) is None         # (16, 64]: lost
    assert gemm.w8_plan(65, 6144, 4096, 0) is None         # above the kernel's M
    assert gemm.w8_plan(4, 6144, 4096, 1) is None          # another epilogue: no row
    assert gemm.w8_plan(4, 4096, 4096, 0) is None          # another shape: no row
    assert gemm.w8a16_step_ok(4, ((6144, 4096, 0),)) and not gemm.w8a16_step_ok(4, ((6144, 4096, 0), (4096, 4096, 2)))
    gemm.W8_SKINNY = "off"                                  # the switch drops the cached picks
    assert gemm.w8_plan(3, 6144, 4096, 0) is None
    gemm.W8_SKINNY = "model"
    assert gemm.w8_plan(4, 4096, 4096, 0) is not None
    gemm.W8_SKINNY = "plan"
    assert gemm.w8_plan(3, 6144, 4096, 0) == (0, 1) and gemm.w8_plan(4, 4096, 4096, 0) is None
    # a routed row that is not valid for its M is today's route instead of reaching the binding
    _load(gemm, monkeypatch, tmp_path, {"w8plans": {"6144,4096,0": [[32, 0, 1]]}})
    assert gemm.w8_plan(16, 6144, 4096, 0) == (0, 1) and gemm.w8_plan(17, 6144, 4096, 0) is None


@pytest.mark.parametrize("value", ["plan", "off"])
def test_missing_section_and_off_are_todays_route_everywhere(gemm, monkeypatch, tmp_path, value):
    gemm.W8_SKINNY = value
    raw = {"plans": {"6144,4096,0": [[64, 101, 1]]}}
    if value == "off":
        raw["w8plans"] = {f"{n},{k},{mode}": [[64, 0, 1]] for n, k, mode in SHAPES_8B}
    _load(gemm, monkeypatch, tmp_path, raw)
    for m, (n, k, mode) in itertools.product((2, 3, 5, 16, 64), SHAPES_8B):
        assert gemm.w8_plan(m, n, k, mode) is None
        assert not gemm.w8a16_step_ok(max(m, 3), SHAPES_8B)
    assert not gemm.resid_ok_a16(5, 4096, 4096)
    assert gemm.resid_ok_a16(1, 4096, 4096) == gemm.resid_ok(1, 4096, 4096, True)


def _binding_accepts(cfg, m, n, k, mode, sk, table):
    """csrc/kernels/bindings.cpp gemm_skinny with ``wscale``, written out independently of ops/gemm.py."""
    if not 0 <= cfg < len(table):
        return False
    rt, mt, nw = table[cfg]
    if not 1 <= m <= 16 * mt:
        return False
    if sk < 1 or k % (64 * nw * sk) != 0 or k > 1 << 20:
        return False
    if mode == 1:
        return rt % 2 == 0 and n % 2 == 0 and (n // 2) % (8 * rt) == 0
    return n % (16 * rt) == 0


def test_validity_predicate_matches_the_binding(gemm):
    table = gemm._SK8
    assert sorted(table) == list(range(len(table))) and len(table) <= 13
    assert all(mt in (1, 2, 4) for _, mt, _ in table.values())  # M <= 16 MT <= 64
    ms = (0, 1, 3, 16, 17, 32, 33, 64, 65)
    ns = (16, 32, 48, 64, 96, 512, 1024, 1536, 4096, 5632, 6144, 28672)
    ks = (64, 128, 512, 1024, 1536, 2048, 2816, 4096, 6144, 14336)
    n_ok = 0
    for cfg, m, n, k, mode, sk in itertools.product(range(-1, len(table) + 1), ms, ns, ks, (0, 1, 2), (1, 2, 3, 7, 8)):
        want = _binding_accepts(cfg, m, n, k, mode, sk, table)
        assert gemm._sk8_valid(cfg, m, n, k, mode, sk) == want, (cfg, m, n, k, mode, sk)
        n_ok += want
    assert n_ok > 1000
    # the 8B shapes and the small preset's four projections (K = 2816 included) are reachable at every MT
    for mt in (1, 2, 4):
        for n, k, mode in SHAPES_8B + SMALL:
            assert any(gemm._sk8_valid(c, 16 * mt, n, k, mode, 1) for c in table if table[c][1] == mt), (mt, n, k)
            pick = gemm._sk8_model(16 * mt, n, k, mode)
            assert pick is not None and gemm._sk8_valid(pick[0], 16 * mt, n, k, mode, pick[1])


def test_committed_rows_are_valid(gemm):
    with open(os.path.join(os.path.dirname(os.path.abspath(gemm.__file__)), "gemm_plan.json")) as fh:
        raw = json.load(fh)
    assert "w8plans" in raw
    for key, rows in raw["w8plans"].items():
        n, k, mode = (int(v) for v in key.split(","))
        assert [r[0] for r in rows] == sorted({r[0] for r in rows})
        for m, cfg, sk in rows:
            assert 1 <= m <= 64, (key, m)
            assert cfg < 0 or gemm._sk8_valid(cfg, m, n, k, mode, sk), (key, m, cfg, sk)


def test_committed_rows_follow_the_measured_table(gemm):
    """A routed row is the table's best config at that M, more than 3 % faster than ``qlinear`` alone (M = 2: the W8A16
    GEMV) by more than both spreads; every other measured point is a recorded loss."""
    with open(os.path.join(os.path.dirname(os.path.abspath(gemm.__file__)), "gemm_plan.json")) as fh:
        plans = json.load(fh)["w8plans"]
    with open(TABLE) as fh:
        recs = [json.loads(line) for line in fh if line.strip()]
    assert recs and {(r["N"], r["K"], r["mode"]) for r in recs} == set(SHAPES_8B)
    for r in recs:
        rows = {m: (cfg, sk) for m, cfg, sk in plans[f"{r['N']},{r['K']},{r['mode']}"]}
        spread = (r["w8_spread_us"][1] - r["w8_spread_us"][0]) + (r["today_spread_us"][1] - r["today_spread_us"][0])
        won = r["w8_us"] < 0.97 * r["today_us"] and r["today_us"] - r["w8_us"] > spread
        assert won == r["w8_wins"]
        assert rows[r["M"]] == ((r["w8_cfg"], r["w8_splitk"]) if won else (-1, 1)), (r["kind"], r["M"])
        assert r["today"] == ("w8a16_gemv" if r["M"] <= 2 else "qlinear")


@pytest.mark.parametrize("value", ["plan", "off", "model"])
def test_cpu_qtensors_unchanged(gemm, value):
    from chronos import ops
    from chronos.models.llama import QTensor
    from chronos.ops import reference as ref

    g = torch.Generator().manual_seed(3)
    wq, ws = ref.quantize_weight((torch.randn(512, 1024, generator=g) * 0.02).to(torch.bfloat16))
    w8 = QTensor(wq.contiguous(), ws.contiguous())
    xs = [torch.randn(m, 1024, generator=g).to(torch.bfloat16) for m in (1, 4, 20)]
    gemm.W8_SKINNY = "off"
    want = [(ops.linear(x, w8), ops.gate_up_silu(x, w8)) for x in xs]
    gemm.W8_SKINNY = value
    before = dict(gemm.w8_stats)
    for x, (y, h) in zip(xs, want):
        for a16 in (False, True):
            assert torch.equal(ops.linear(x, w8, a16=a16), y)
            assert torch.equal(ops.gate_up_silu(x, w8, a16=a16), h)
    assert gemm.w8_stats == before


def test_default_calls_log_what_they_log_today_and_a16_reaches_the_kernel(gemm):
    import _gemm_dispatch as D

    with open(D.GOLDEN) as fh:
        golden = json.load(fh)

    def today(case, m):
        return next(golden["logs"][i] for lo, hi, i in golden["cases"][case] if lo <= m <= hi)

    ms = (1, 2, 3, 4, 5, 16, 17, 33, 64, 65, 128)
    for value in ("plan", "model"):
        gemm.W8_SKINNY = value
        gemm._plan_cache.clear()
        with D.harness() as rec:
            for n, k, mode in SHAPES_8B:
                w = D.make_weight(rec, "fp8", n, k)
                for entry in D.ENTRIES[mode]:
                    if entry == "qkv_rope":
                        continue
                    for xkind in D._xkinds(entry):
                        for m in ms:
                            got = D.run_one(rec, entry, w, xkind, m, n, k)
                            assert got == today(f"{entry}|{n},{k},{mode}|fp8|{xkind}|default", m), (value, entry, m)
    # a16 under ``model``: one gemm_skinny with the row scales as ``wscale``, at every M = 3..64
    gemm.W8_SKINNY = "model"
    gemm._plan_cache.clear()
    from chronos import ops

    with D.harness() as rec:
        for n, k, mode in SHAPES_8B:
            w = D.make_weight(rec, "fp8", n, k)
            for xkind in (("plain",) if mode == 2 else ("plain", "lazy")):
                for m in range(1, 70):
                    x = D.make_x(rec, xkind, m, k)
                    rec.begin()
                    c0 = gemm.w8_stats["skinny_launches"]
                    if mode == 2:
                        if not ops.resid_ok_a16(m, n, k):
                            assert not 3 <= m <= 64
                            continue
                        out = ops.gemv_resid(x, w, rec.operand("resid", (m, n)), a16=True)
                        assert isinstance(out, ops.ResidOut)
                    elif mode == 1:
                        ops.gate_up_silu(x, w, a16=True)
                    else:
                        ops.linear(x, w, a16=True)
                    names = [c[0] for c in rec.log]
                    if 3 <= m <= 64:
                        assert names == ["gemm_skinny"], (n, k, mode, xkind, m, names)
                        call = rec.log[0]
                        cfg, sk = gemm.w8_plan(m, n, k, mode)
                        assert call[1] == ("s" if xkind == "lazy" else "x") and call[2] == "q8"
                        assert call[3:6] == [mode, cfg, sk]
                        assert call[7] == ("part" if xkind == "lazy" else None)  # the folded norm as the prologue
                        assert call[9] is None and call[10] == "ws"            # we absent, wscale = the row scales
                        assert gemm.w8_stats["skinny_launches"] == c0 + 1
                    else:
                        assert "gemm_skinny" not in names and gemm.w8_stats["skinny_launches"] == c0


def test_engine_config_default(monkeypatch):
    from chronos.brain.engine.engine import EngineConfig

    monkeypatch.delenv("CHRONOS_W8A16_ROWS", raising=False)
    assert EngineConfig().fp8_a16_rows == 2
    monkeypatch.setenv("CHRONOS_W8A16_ROWS", "48")  # the scripts' way to move the default
    assert EngineConfig().fp8_a16_rows == 48 and EngineConfig(fp8_a16_rows=3).fp8_a16_rows == 3
