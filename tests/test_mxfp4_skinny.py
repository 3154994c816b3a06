"""Routing of the W4A16 skinny GEMM (ops/gemm.py w4_plan): the "w4plans" section of gemm_plan.json, the validity
predicate against the binding's rules, the committed rows against the measured table, and the CPU path."""
import itertools
import json
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "profiles", "mxfp4", "skinny_table.jsonl")


@pytest.fixture
def gemm():
    """ops/gemm.py with its plan tables, cache and switch restored afterwards."""
    from chronos.ops import gemm as g

    old = g.W4_SKINNY
    try:
        yield g
    finally:
        g.W4_SKINNY = old
        g._reset_plans()


def _load(gemm, monkeypatch, tmp_path, raw):
    path = tmp_path / "plan.json"
    path.write_text(json.dumps(raw))
    monkeypatch.setenv("CHRONOS_GEMM_PLAN", str(path))
    gemm._reset_plans()


def test_w4plans_section_parses(gemm, monkeypatch, tmp_path):
    gemm.W4_SKINNY = "plan"
    _load(gemm, monkeypatch, tmp_path, {"plans": {}, "w4plans": {"6144,4096,0": [[2, -1, 1], [5, 0, 1], [16, 2, 2],
                                                                                  [64, -1, 1]]}})
    assert gemm.w4_plan(2, 6144, 4096, 0) is None          # cfg < 0: the copy
    assert gemm.w4_plan(3, 6144, 4096, 0) == (0, 1)        # (2, 5]
    assert gemm.w4_plan(5, 6144, 4096, 0) == (0, 1)
    assert gemm.w4_plan(8, 6144, 4096, 0) == (2, 2)        # (5, 16]
    assert gemm.w4_plan(17, 6144, 4096, 0) is None         # (16, 64]: the copy; cfg 2 has MT = 1 anyway
    assert gemm.w4_plan(65, 6144, 4096, 0) is None         # above the kernel's M
    assert gemm.w4_plan(4, 6144, 4096, 1) is None          # another epilogue: no row
    assert gemm.w4_plan(4, 4096, 4096, 0) is None          # another shape: no row
    gemm.W4_SKINNY = "off"                                  # the switch drops the cached picks
    assert gemm.w4_plan(3, 6144, 4096, 0) is None
    gemm.W4_SKINNY = "model"
    assert gemm.w4_plan(4, 4096, 4096, 0) is not None
    gemm.W4_SKINNY = "plan"
    assert gemm.w4_plan(3, 6144, 4096, 0) == (0, 1) and gemm.w4_plan(4, 4096, 4096, 0) is None
    # a routed row that is not valid for its M falls back to the copy instead of reaching the binding
    _load(gemm, monkeypatch, tmp_path, {"w4plans": {"6144,4096,0": [[32, 0, 1]]}})
    assert gemm.w4_plan(16, 6144, 4096, 0) == (0, 1) and gemm.w4_plan(17, 6144, 4096, 0) is None


def test_missing_section_is_the_copy_everywhere(gemm, monkeypatch, tmp_path):
    gemm.W4_SKINNY = "plan"
    _load(gemm, monkeypatch, tmp_path, {"plans": {"6144,4096,0": [[64, 101, 1]]}})
    for m, (n, k, mode) in itertools.product((2, 3, 5, 16, 64), ((6144, 4096, 0), (4096, 4096, 2), (28672, 4096, 1),
                                                                   (4096, 14336, 2))):
        assert gemm.w4_plan(m, n, k, mode) is None


def _binding_accepts(cfg, m, n, k, mode, sk, table):
    """csrc/kernels/bindings.cpp gemm_skinny with ``we``, written out independently of ops/gemm.py."""
    if not 0 <= cfg < len(table):
        return False
    rt, mt, nw = table[cfg]
    if not 1 <= m <= 16 * mt:
        return False
    if sk < 1 or k % (128 * nw * sk) != 0 or k > 1 << 20:
        return False
    if mode == 1:
        return rt % 2 == 0 and n % 2 == 0 and (n // 2) % (8 * rt) == 0
    return n % (16 * rt) == 0


def test_validity_predicate_matches_the_binding(gemm):
    table = gemm._SK4
    assert sorted(table) == list(range(len(table)))
    ms = (0, 1, 3, 16, 17, 32, 33, 64, 65)
    ns = (16, 32, 48, 64, 96, 512, 4096, 5632, 6144, 28672)
    ks = (128, 512, 1024, 1536, 2048, 2816, 4096, 6144, 14336)
    n_ok = 0
    for cfg, m, n, k, mode, sk in itertools.product(range(-1, len(table) + 1), ms, ns, ks, (0, 1, 2), (1, 2, 3, 7, 8)):
        want = _binding_accepts(cfg, m, n, k, mode, sk, table)
        assert gemm._sk4_valid(cfg, m, n, k, mode, sk) == want, (cfg, m, n, k, mode, sk)
        n_ok += want
    assert n_ok > 1000
    # both 8B K are reachable at every MT, in every epilogue
    for mt in (1, 2, 4):
        for n, k, mode in ((6144, 4096, 0), (4096, 4096, 2), (28672, 4096, 1), (4096, 14336, 2)):
            assert any(gemm._sk4_valid(c, 16 * mt, n, k, mode, 1) for c in table if table[c][1] == mt), (mt, n, k)
            assert gemm._sk4_model(16 * mt, n, k, mode) is not None


def test_committed_rows_are_valid_and_measured(gemm):
    with open(os.path.join(os.path.dirname(os.path.abspath(gemm.__file__)), "gemm_plan.json")) as fh:
        raw = json.load(fh)
    assert "w4plans" in raw
    with open(TABLE) as fh:
        recs = [json.loads(line) for line in fh if line.strip()]
    assert recs
    by = {(r["N"], r["K"], r["mode"], r["M"]): r for r in recs}
    for key, rows in raw["w4plans"].items():
        n, k, mode = (int(v) for v in key.split(","))
        assert [r[0] for r in rows] == sorted({r[0] for r in rows})
        for m, cfg, sk in rows:
            rec = by.get((n, k, mode, m))
            assert rec is not None, (key, m)
            if cfg < 0:  # a measured loss: the copy
                assert not rec["w4_wins"], (key, m)
                continue
            assert gemm._sk4_valid(cfg, m, n, k, mode, sk), (key, m, cfg, sk)
            assert (cfg, sk) == (rec["w4_cfg"], rec["w4_splitk"]), (key, m)
            assert rec["w4_us"] < 0.97 * rec["bf16_routed_us"], (key, m, rec["w4_us"], rec["bf16_routed_us"])
            spread = (rec["w4_spread_us"][1] - rec["w4_spread_us"][0]) + \
                (rec["bf16_spread_us"][1] - rec["bf16_spread_us"][0])
            assert rec["bf16_routed_us"] - rec["w4_us"] > spread, (key, m)
    # and nothing the table shows as a win is missing a row of its own
    for r in recs:
        rows = raw["w4plans"].get(f"{r['N']},{r['K']},{r['mode']}", [])
        if r["w4_wins"]:
            assert [r["M"], r["w4_cfg"], r["w4_splitk"]] in rows, r


@pytest.mark.parametrize("value", ["plan", "off", "model"])
def test_cpu_q4tensors_unchanged(gemm, value):
    from chronos import ops
    from chronos.models.llama import quantize_mxfp4

    gemm.W4_SKINNY = value
    g = torch.Generator().manual_seed(3)
    w4 = quantize_mxfp4((torch.randn(512, 1024, generator=g) * 0.02).to(torch.bfloat16))
    before = dict(gemm.w4_stats)
    for m in (1, 4, 20):
        x = torch.randn(m, 1024, generator=g).to(torch.bfloat16)
        assert torch.equal(ops.linear(x, w4), ops.linear(x, w4.w))
        assert torch.equal(ops.gate_up_silu(x, w4), ops.gate_up_silu(x, w4.w))
    assert gemm.w4_stats == before
