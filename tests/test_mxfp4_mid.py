"""Mid-M W4A16 GEMM (csrc/kernels/gemm_w4m.hip, ops/gemm.py ``w4m_plan``), CPU side: the ``encode_pm1`` builder of
tests/_w4m_probes.py proved against ``ops.reference.dequantize_mxfp4``, the mutations the integer probes notice, the
"w4mplans" section of gemm_plan.json, the validity predicate and the cost model, the committed rows against the measured
table, and the CPU path."""
import itertools
import json
import os

import pytest
import torch

import _gemm_probes as P
import _w4m_probes as W
from _mxfp4_cases import codes_of, pack

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "profiles", "mxfp4", "mid_table.jsonl")
SHAPES_8B = ((6144, 4096, 0), (4096, 4096, 2), (28672, 4096, 1), (4096, 14336, 2))
BUILDER_SHAPES = ((192, 384), (130, 1024), (64, 4096), (96, 1792))


def _deq(q, e):
    from chronos.ops import reference as ref

    return ref.dequantize_mxfp4(q, e)


def _y(x, q, e):
    """x dequant(q, e)^T in fp64: integers on the unmutated probes."""
    return x.double() @ _deq(q, e).double().t()


# ---- the builder ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,k", BUILDER_SHAPES)
def test_encode_pm1_is_exact_and_scale_sensitive(n, k):
    w, q, e = W.make_w4(n, k, 11 * n + k)
    assert q.shape == (n, k // 2) and e.shape == (n, k // 32) and q.dtype == e.dtype == torch.uint8
    d = _deq(q, e)
    assert d.dtype == torch.bfloat16 and torch.equal(d.view(torch.int16), w.view(torch.int16))  # bit for bit, -0 never
    assert sorted(e.unique().tolist()) == sorted(W.CLASS_E)                                   # all four classes occur
    cls = W.block_classes(n, k // 32, 11 * n + k + 5)
    assert bool((cls[1:] != cls[:-1]).all()) and bool((cls[:, 1:] != cls[:, :-1]).all())       # neighbours differ
    assert int((w.view(n, k // 32, 32) != 0).sum(-1).min()) == 1 and int((w != 0).sum(1).max()) == k // 32
    x = P.make_x(24, k, 3)
    y = _y(x, q, e)
    assert torch.equal(y, P.expect_plain(x, w)) and float(y.abs().max()) <= 2 * k / 32 <= 256
    # the scale bytes of blocks 0 and 1 exchanged: every output column (W row) changes
    e2 = e.clone()
    e2[:, 0], e2[:, 1] = e[:, 1], e[:, 0]
    assert bool((_y(x, q, e2) != y).any(0).all())
    # the nibbles of every byte exchanged: k and k ^ 1 trade places under every non-zero
    qs = ((q >> 4) | (q << 4)).to(torch.uint8)
    frac = float((_y(x, qs, e) != y).float().mean())
    print(f"nibble exchange changes {100 * frac:.1f} % of the outputs")
    assert frac > 0.9


def test_encode_pm1_default_group_above_4096():
    w, q, e = W.make_w4(48, 8192, 2)
    assert W.probe_g(8192) is None and torch.equal(_deq(q, e).view(torch.int16), w.view(torch.int16))
    assert float(P.expect_plain(P.make_x(8, 8192, 1), w).abs().max()) <= 128


# ---- mutations the probes notice -----------------------------------------------------------------------------------


def _tiles_differ(y, e, wn, xm):
    """[tiles of x rows, tiles of W rows] bool: the output tile holds at least one wrong element."""
    bad = (y != e)
    m, n = bad.shape
    pad = torch.zeros(-(-m // xm) * xm, -(-n // wn) * wn, dtype=torch.bool)
    pad[:m, :n] = bad
    return pad.view(pad.shape[0] // xm, xm, pad.shape[1] // wn, wn).any(3).any(1)


@pytest.mark.parametrize("wn,xm", [(64, 64), (128, 128)])
def test_mutations_show_in_every_tile_they_touch(wn, xm):
    m, n, k = xm + 1, 3 * wn, 128 * 6
    x = P.make_x(m, k, 5)
    w, q, e = W.make_w4(n, k, 6)
    want = P.expect_plain(x, w)
    assert torch.equal(_y(x, q, e), want)
    every = torch.ones(2, 3, dtype=torch.bool)

    def tiles(q2, e2, x2=x):
        return _tiles_differ(_y(x2, q2, e2), want, wn, xm)

    # the last tile of x rows holds one row: an x element is 0 with probability 1 / 5, so a mutation of a few k may
    # miss it; everything that moves a whole block of every W row must show there too
    e2 = e.clone()
    e2[:, 2], e2[:, 3] = e[:, 3], e[:, 2]                        # scale bytes of neighbouring blocks
    assert torch.equal(tiles(q, e2), every)
    e2 = e.clone()
    e2[0::2], e2[1::2] = e[1::2], e[0::2]                        # ... of neighbouring rows
    assert torch.equal(tiles(q, e2), every)
    assert torch.equal(tiles(((q >> 4) | (q << 4)).to(torch.uint8), e), every)  # nibbles exchanged
    q2 = q.clone()
    q2[wn:2 * wn, 16 * 7:16 * 8] = 0                             # one 16-B piece (MX block 7) of the middle W tile
    got = tiles(q2, e)
    assert bool(got[0, 1]) and not bool(got[:, 0].any()) and not bool(got[:, 2].any())
    xs = x.clone()
    xs[:, 128 * 4:128 * 5] = 0                                   # a dropped 128-k stage
    assert torch.equal(tiles(q, e, xs), every)
    xs = x.clone()
    xs[:, k // 3:2 * k // 3] = 0                                 # a dropped split-K slice (of 3)
    assert torch.equal(tiles(q, e, xs), every)
    xs = x.clone()
    xs[:xm, k // 2:] = 0                                         # ... of the first x tile alone
    got = tiles(q, e, xs)
    assert bool(got[0].all()) and not bool(got[1].any())


# ---- routing -------------------------------------------------------------------------------------------------------


@pytest.fixture
def gemm():
    """ops/gemm.py with its plan tables, cache and switches restored afterwards."""
    from chronos.ops import gemm as g

    old = (g.W4_MID, g.W4_SKINNY, g._W4A16_DECODE)
    try:
        yield g
    finally:
        g.W4_MID, g.W4_SKINNY, g._W4A16_DECODE = old
        g._reset_plans()


def _load(gemm, monkeypatch, tmp_path, raw):
    path = tmp_path / "plan.json"
    path.write_text(json.dumps(raw))
    monkeypatch.setenv("CHRONOS_GEMM_PLAN", str(path))
    gemm._reset_plans()


def test_w4mplans_section(gemm, monkeypatch, tmp_path):
    gemm.W4_MID = "plan"
    rows = [[65, 0, 2, 2], [96, 2, 1, 1], [128, 2, 2, 2], [256, -1, 1, 0], [384, 3, 1, 1]]
    _load(gemm, monkeypatch, tmp_path, {"plans": {}, "w4mplans": {"6144,4096,0": rows}})
    plan = lambda m, packed=False, key=(6144, 4096, 0): gemm.w4m_plan(m, *key, packed)  # noqa: E731
    assert plan(64) is None and plan(64, True) is None      # the skinny kernel's range
    assert plan(65) == (0, 2) and plan(65, True) == (0, 2)  # beats 2: both weight modes
    assert plan(66) is None and plan(66, True) == (2, 1)    # (65, 96], beats 1: packed-only tensors alone
    assert plan(96) is None and plan(96, True) == (2, 1)
    assert plan(97) == (2, 2) and plan(128, True) == (2, 2)
    assert plan(129) is None and plan(256, True) is None    # cfg < 0: measured, lost to both
    assert plan(300) is None and plan(300, True) == (3, 1)
    assert plan(385) is None and plan(385, True) is None    # above the last measured M: never measured
    assert plan(512, True) is None and plan(513, True) is None and plan(4096, True) is None
    assert plan(100, True, (6144, 4096, 1)) is None         # another epilogue: no row
    assert plan(100, True, (4096, 4096, 0)) is None         # another shape: no row, and no model pick either
    gemm.W4_MID = "off"                                      # the switch drops the cached picks
    assert plan(65) is None and plan(100, True) is None
    gemm.W4_MID = "model"
    assert plan(100, False, (4096, 4096, 0)) is not None and plan(100, True, (1024, 2816, 2)) is not None
    assert plan(64) is None and plan(513) is None
    gemm._W4A16_DECODE = False
    assert plan(100, True, (4096, 4096, 0)) is None
    gemm._W4A16_DECODE = True
    gemm.W4_MID = "plan"
    assert plan(65) == (0, 2) and plan(100, True, (4096, 4096, 0)) is None
    gemm._W4A16_DECODE = False
    assert plan(65) is None and plan(65, True) is None
    gemm._W4A16_DECODE = True
    # rows the binding would reject fall back to None instead of reaching it: an unknown config, a split-K that does
    # not divide K / 128, a W tile that does not divide N
    _load(gemm, monkeypatch, tmp_path, {"w4mplans": {"6144,4096,0": [[128, 99, 1, 2], [256, 0, 3, 2]],
                                                       "192,4096,0": [[128, 1, 1, 2]]}})
    assert plan(100) is None and plan(200, True) is None and plan(100, True, (192, 4096, 0)) is None
    # W4_SKINNY is a switch of its own
    gemm.W4_SKINNY = "model"
    assert plan(100, True, (4096, 4096, 0)) is None and gemm.w4_plan(80, 4096, 4096, 0, True) is None


def test_missing_section_routes_nothing(gemm, monkeypatch, tmp_path):
    gemm.W4_MID = "plan"
    _load(gemm, monkeypatch, tmp_path, {"plans": {"6144,4096,0": [[128, 39, 1]]}, "w4plans": {"6144,4096,0": [[64, 0, 1]]}})
    for m, (n, k, mode), packed in itertools.product((65, 128, 244, 512), SHAPES_8B + ((1024, 2816, 2),), (False, True)):
        assert gemm.w4m_plan(m, n, k, mode, packed) is None


def _binding_accepts(cfg, m, n, k, mode, sk, table):
    """csrc/kernels/bindings.cpp gemm_w4m, written out independently of ops/gemm.py."""
    if not 0 <= cfg < len(table):
        return False
    wn = table[cfg][0]
    if m < 1 or k < 1 or k > 1 << 20 or m * k >= 1 << 30 or k % 32:
        return False
    if sk < 1 or k % (128 * sk) != 0:
        return False
    if mode == 1:
        return n % 2 == 0 and (n // 2) % (wn // 2) == 0
    return n % wn == 0


def test_validity_predicate_and_model(gemm):
    table = gemm._W4M
    assert sorted(table) == list(range(len(table))) and len(table) <= 8
    assert (gemm.W4M_MIN_M, gemm.W4M_MAX_M) == (gemm.W4_SKINNY_MAX_M + 1, 512)
    ms = (0, 1, 65, 128, 244, 512, 513, 300000)
    ns = (32, 64, 96, 128, 192, 1024, 1536, 4096, 5632, 6144, 28672)
    ks = (96, 128, 384, 1024, 2816, 4096, 14336)
    n_ok = 0
    for cfg, m, n, k, mode, sk in itertools.product(range(-1, len(table) + 1), ms, ns, ks, (0, 1, 2), (0, 1, 2, 3, 8)):
        want = _binding_accepts(cfg, m, n, k, mode, sk, table)
        assert gemm._w4m_valid(cfg, m, n, k, mode, sk) == want, (cfg, m, n, k, mode, sk)
        n_ok += want
    assert n_ok > 1000
    picked = set()
    for (n, k, mode), m in itertools.product(SHAPES_8B, (65, 80, 96, 128, 192, 256, 384, 512)):
        for cfg in table:  # every config reaches every 8B projection at some split-K
            assert any(gemm._w4m_valid(cfg, m, n, k, mode, sk) for sk in (1, 2, 4, 7, 8)), (cfg, n, k)
        pick = gemm._w4m_model(m, n, k, mode)
        assert pick is not None and gemm._w4m_valid(pick[0], m, n, k, mode, pick[1])
        picked.add(pick[0])
    for (n, k, mode), m in itertools.product(((1536, 1024, 0), (1024, 1024, 2), (5632, 1024, 1), (1024, 2816, 2)),
                                             (80, 244)):  # "small": K = 2816 = 128 * 22 is accepted
        pick = gemm._w4m_model(m, n, k, mode)
        assert pick is not None and gemm._w4m_valid(pick[0], m, n, k, mode, pick[1])
        picked.add(pick[0])
    assert picked == set(table), picked  # no compiled config that the model never picks on these shapes
    assert gemm._w4m_model(100, 100, 4096, 0) is None and gemm._w4m_model(100, 4096, 4000, 0) is None


def test_committed_rows_are_valid_and_measured(gemm):
    with open(os.path.join(os.path.dirname(os.path.abspath(gemm.__file__)), "gemm_plan.json")) as fh:
        raw = json.load(fh)
    assert "w4mplans" in raw and "w4mplans" in raw["meta"]
    with open(TABLE) as fh:
        recs = [json.loads(line) for line in fh if line.strip()]
    assert recs
    by = {(r["N"], r["K"], r["mode"], r["M"]): r for r in recs}
    assert {(r["N"], r["K"], r["mode"]) for r in recs} == set(SHAPES_8B)
    assert {r["M"] for r in recs} == {65, 80, 96, 128, 192, 256, 384, 512}
    spread = lambda r, a, b: (r[a][1] - r[a][0]) + (r[b][1] - r[b][0])  # noqa: E731

    def beats(r):
        """The project's win rule (tests/test_mxfp4_skinny.py) against the copy's kernel, then against the expansion."""
        if r["w4m_us"] < 0.97 * r["bf16_routed_us"] and \
                r["bf16_routed_us"] - r["w4m_us"] > spread(r, "w4m_spread_us", "bf16_spread_us"):
            return 2
        if r["w4m_us"] < 0.97 * r["expand_us"] and \
                r["expand_us"] - r["w4m_us"] > spread(r, "w4m_spread_us", "expand_spread_us"):
            return 1
        return 0

    for key, rows in raw["w4mplans"].items():
        n, k, mode = (int(v) for v in key.split(","))
        assert [r[0] for r in rows] == sorted({r[0] for r in rows})
        for m, cfg, sk, b in rows:
            rec = by.get((n, k, mode, m))
            assert rec is not None, (key, m)
            assert rec["expand_us"] > rec["bf16_routed_us"] * 0.97, (key, m)  # the expansion is not free
            assert b == beats(rec) == rec["beats"], (key, m, b, beats(rec))
            if cfg < 0:  # a measured loss to both
                assert b == 0, (key, m)
                continue
            assert b in (1, 2) and gemm._w4m_valid(cfg, m, n, k, mode, sk), (key, m, cfg, sk)
            assert (cfg, sk) == (rec["w4m_cfg"], rec["w4m_splitk"]), (key, m)
    for r in recs:  # every measured point has its row, wins and losses alike
        rows = raw["w4mplans"].get(f"{r['N']},{r['K']},{r['mode']}", [])
        b = beats(r)
        want = [r["M"], r["w4m_cfg"], r["w4m_splitk"], b] if b else [r["M"], -1, 1, 0]
        assert want in rows, (r["N"], r["K"], r["mode"], r["M"], want)
        assert r["screen"] and all(v > 0 for v in r["screen"].values())


@pytest.mark.parametrize("value", ["plan", "off", "model"])
def test_cpu_q4tensors_unchanged(gemm, value):
    from chronos import ops
    from chronos.models.llama import quantize_mxfp4

    gemm.W4_MID = value
    g = torch.Generator().manual_seed(3)
    w4 = quantize_mxfp4((torch.randn(512, 1024, generator=g) * 0.02).to(torch.bfloat16))
    wd = quantize_mxfp4((torch.randn(1024, 512, generator=g) * 0.02).to(torch.bfloat16))
    before = dict(gemm.w4_stats)
    assert "mid_launches" in before
    x = torch.randn(80, 1024, generator=g).to(torch.bfloat16)
    assert torch.equal(ops.linear(x, w4), ops.linear(x, w4.w))
    assert torch.equal(ops.gate_up_silu(x, w4), ops.gate_up_silu(x, w4.w))
    assert torch.equal(ops.linear(x[:, :512].contiguous(), wd), ops.linear(x[:, :512].contiguous(), wd.w))
    assert gemm.w4_stats == before


def test_pack_roundtrip_of_the_probe_codes():
    w, q, e = W.make_w4(32, 256, 9)
    c = codes_of(q)
    assert torch.equal(pack(c), q) and set(c.unique().tolist()) <= {0, 1, 2, 4, 6, 9, 10, 12, 14}
