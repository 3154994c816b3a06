"""CPU half of the projection-GEMM probes (tests/_gemm_probes.py): the builders have the properties the GPU tests rely
on, every mutation a software-pipelined tile GEMM can suffer is noticed in every output tile it touches, and the GPU
file's config lists are the op's full tables."""
import pytest
import torch

import _gemm_probes as P

SHAPES = [(17, 52, 64), (33, 36, 640), (33, 200, 1024), (32, 300, 4096), (32, 500, 14336)]


def _ids(s):
    return "M{}-N{}-K{}".format(*s)


# ---- builder proofs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_operands_are_small_integers(shape):
    m, n, k = shape
    x, w, r = P.make_x(m, k, 1), P.make_w(n, k, 2), P.make_resid(m, n, 3)
    assert x.dtype == w.dtype == r.dtype == torch.bfloat16
    assert set(x.float().unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert set(w.float().unique().tolist()) == {-1.0, 0.0, 1.0}
    rf = r.float()
    assert torch.equal(rf, rf.round()) and rf.abs().max() <= 64 and rf.abs().max() >= 60
    rq = P.make_resid(m, n, 3, frac=True).float() * 64
    assert torch.equal(rq, rq.round()) and rq.abs().max() <= 127


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_w_blocks_are_signed_permutations(shape):
    _, n, k = shape
    g = P.group(k)
    assert g == max(16, k // 64) and k % g == 0 and n % g != 0
    w = P.make_w(n, k, 2).float()
    assert torch.equal(w.abs().sum(1), torch.full((n,), float(k // g)))  # K / G non-zeros per row
    full = n // g * g
    blk = w[:full].view(n // g, g, k // g, g).abs()
    assert torch.equal(blk.sum(1), torch.ones(n // g, k // g, g))  # every k once per row group
    assert torch.equal(blk.sum(3), torch.ones(n // g, g, k // g))  # every row once per k block
    tail = w[full:].view(n - full, k // g, g).abs()  # the last group keeps only its own rows
    assert torch.equal(tail.sum(2), torch.ones(n - full, k // g)) and tail.sum(0).max() <= 1
    assert (w == 1).sum() > 0 and (w == -1).sum() > 0
    # two seeds give different matrices (the repeat-call check depends on it)
    assert not torch.equal(w, P.make_w(n, k, 3).float())


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_expectations_are_exact(shape):
    m, n, k = shape
    x, w, r = P.make_x(m, k, 1), P.make_w(n, k, 2), P.make_resid(m, n, 3)
    e = P.expect_plain(x, w)
    assert torch.equal(e, e.round()) and e.abs().max() <= 128 and e.abs().max() <= 2 * k // P.group(k)
    # the int64 product, and a bf16-operand fp32 matmul, give the same bits
    assert torch.equal(e, (x.long() @ w.long().t()).double())
    assert torch.equal(e.float(), x.float() @ w.float().t())
    assert torch.equal(e.to(torch.bfloat16).double(), e)
    s, ss = P.expect_resid(x, w, r)
    assert torch.equal(s.double(), e + r.double()) and s.double().abs().max() <= 192
    # every partial (<= 256 columns) is an integer below 2^24: exact in fp32 in any order
    pad = (-n) % 256
    sq = torch.nn.functional.pad(s.double() ** 2, (0, pad)).view(m, -1, 256).sum(-1)
    assert sq.max() < 2 ** 24 and 256 * 192 ** 2 < 2 ** 24
    assert torch.equal(ss, (s.long() ** 2).sum(1).double())


@pytest.mark.parametrize("k", [64, 640, 1024, 4096])
def test_swiglu_gate_rows(k):
    f, m = 40, 33
    w = P.make_w_swiglu(f, k, 5)
    assert torch.equal(w[:f].float().abs().sum(1), torch.full((f,), 16.0))
    x = P.make_x(m, k, 6)
    h = P.expect_plain(x, w)
    assert h[:, :f].abs().max() <= 32 and h[:, f:].abs().max() <= 128
    e = P.expect_swiglu(x, w)
    nz = e[e != 0].abs()
    assert nz.min() > 1e-30 and torch.isfinite(e).all()  # silu stays a normal float (bf16's smallest: 1.2e-38)
    # at inv = 2 as well
    e2 = P.expect_swiglu(x, w, torch.full((m, 1), 2.0, dtype=torch.float64))
    assert e2[e2 != 0].abs().min() > 1e-30


@pytest.mark.parametrize("m,k,p", [(1, 512, 128), (33, 640, 16), (257, 4096, 72), (40, 14336, 8)])
def test_parts_builder(m, k, p):
    part = P.make_parts(m, k, p, 9)
    assert part.dtype == torch.float32 and part.shape == (m, p) and (part >= 0).all()
    inv = P.inv_of(part, k).squeeze(1)
    cls = torch.tensor(P.INV_CLASSES, dtype=torch.float64)[P.inv_classes(m, 9)]
    assert ((inv / cls - 1).abs() < 1e-6).all()
    if m > 1:
        ratio = inv[1:] / inv[:-1]
        assert (torch.maximum(ratio, 1 / ratio) > 1.99).all()  # neighbouring rows differ by >= 2x
    cols = (part > 0).sum(1)
    assert cols.min() >= 1 and cols.max() <= 4
    assert (part[torch.arange(m), (p - 1 - torch.arange(m)) % p] > 0).all()  # row 0: the last column
    # what the kernels do with it: the scaled integer, rounded to bf16, is the exact power-of-two multiple
    acc = torch.arange(-256, 257, dtype=torch.float64)[None, :]
    got = (inv[:, None].float() * acc.float()).to(torch.bfloat16).double()
    assert torch.equal(got, cls[:, None] * acc)


def test_carve_poison():
    x = P.make_x(5, 64, 1)
    v = P.carve(x)
    assert torch.equal(v, x) and v.is_contiguous() and v.storage_offset() * 2 % 256 == 0 and P.guard_ok(v)
    base = v.new_empty(0).set_(v.untyped_storage(), 0, (v.numel() + 2 * (P.PAD_BYTES // 2),))
    assert base.isnan().sum() == 2 * (P.PAD_BYTES // 2)
    base[P.PAD_BYTES // 2 - 1] = 0
    assert not P.guard_ok(v)
    f = P.carve(torch.ones(3, 4))
    assert f.dtype == torch.float32 and P.guard_ok(f)
    q = P.carve(P.to_e4m3(x))
    assert q.dtype == torch.uint8 and P.guard_ok(q) and torch.equal(q.view(torch.float8_e4m3fn).float(), x.float())
    assert torch.isnan(torch.tensor([0x7F], dtype=torch.uint8).view(torch.float8_e4m3fn).float()).all()
    # NaN reaches the product through a zero weight
    assert torch.isnan(torch.tensor(float("nan")) * 0)


def test_fp8_scales_exact():
    m, n, k = 33, 132, 256
    x, w = P.make_x(m, k, 1), P.make_w(n, k, 2)
    xs, ws = P.pow2_scales(m), P.pow2_scales(n)
    assert set(xs.tolist()) == {0.5, 1.0, 2.0}
    e = P.expect_plain(x, w) * xs.double()[:, None] * ws.double()[None, :]
    assert torch.equal(e.to(torch.bfloat16).double(), e)  # an integer <= 128 times a power of two: exact in bf16
    assert torch.equal(P.to_e4m3(x).view(torch.float8_e4m3fn).float(), x.float())


# ---- mutations ---------------------------------------------------------------------------------------------------
# Each is applied to the reference computation; ``_col_tiles_hit`` / ``_row_tiles_hit`` then demand that the result
# leaves the expectation by at least 1 (plain / residual) or by twice the bound (SwiGLU, norm prologue) in every tile
# the mutation touches: for a
# k-side mutation every (16 x rows, output column whose W row holds one of the touched k) pair, for a row-side mutation
# every 16-column tile of the row.
MT = 16


def _col_tiles_hit(hit, cols):
    m = hit.shape[0] // MT * MT
    t = hit[:m].view(m // MT, MT, -1).any(1)
    assert cols.any() and bool(t[:, cols].all()), f"{int((~t[:, cols]).sum())} touched tiles unnoticed"


def _row_tiles_hit(hit, row):
    n = hit.shape[1] // MT * MT
    t = hit[row, :n].view(-1, MT).any(1)
    assert bool(t.all()), f"{int((~t).sum())} tiles of row {row} unnoticed"


def _k_mutations(x, k, sk):
    """name -> (x', w-column weights) such that the mutated product is x' @ (w * colw)^T, and the touched k."""
    g = P.group(k)
    out = {}
    k0 = (k // g // 2) * g + (3 if k > 64 else 0)  # inside one G-block
    xz = x.clone()
    xz[:, k0] = 0
    out["x_column_zeroed"] = (xz, None, [k0])
    k8 = (k // g // 3) * g  # an aligned 16-byte piece inside one G-block
    xd = x.clone()
    xd[:, k8:k8 + 8] = 0
    out["k_group_of_8_dropped"] = (xd, None, list(range(k8, k8 + 8)))
    xs = x.clone()
    xs[:, [k0, k0 + 1]] = x[:, [k0 + 1, k0]]
    out["adjacent_k_swapped_in_x"] = (xs, None, [k0, k0 + 1])
    xl = x.clone()
    xl[:, k - 64:] = 0
    out["last_unit_dropped"] = (xl, None, list(range(k - 64, k)))
    cw = torch.ones(k, dtype=torch.float64)
    cw[:64] = 2
    out["first_unit_twice"] = (x, cw, list(range(64)))
    if sk > 1:
        per = k // sk
        xk = x.clone()
        xk[:, per:2 * per] = 0
        out["splitk_slice_dropped"] = (xk, None, list(range(per, 2 * per)))
    return out


@pytest.mark.parametrize("shape,sk", [((32, 52, 64), 1), ((48, 200, 1024), 2), ((32, 300, 4096), 4), ((32, 500, 14336), 7),
                                      ((32, 72, 640), 5)], ids=lambda v: _ids(v) if isinstance(v, tuple) else f"sk{v}")
def test_k_side_mutations_plain(shape, sk):
    m, n, k = shape
    x, w = P.make_x(m, k, 11), P.make_w(n, k, 12)
    e = P.expect_plain(x, w)
    for name, (xm, cw, ks) in _k_mutations(x, k, sk).items():
        wd = w.double() if cw is None else w.double() * cw
        mut = xm.double() @ wd.t()
        cols = (w[:, ks] != 0).any(1)
        _col_tiles_hit((mut - e).abs() >= 1, cols)
        assert torch.equal(mut[:, ~cols], e[:, ~cols]), name


@pytest.mark.parametrize("k,sk", [(64, 1), (640, 2), (1024, 4)])
@pytest.mark.parametrize("normp", [False, True])
def test_k_side_mutations_swiglu(k, sk, normp):
    m, f = 48, 40
    x, w = P.make_x(m, k, 13), P.make_w_swiglu(f, k, 14)
    inv = P.inv_of(P.make_parts(m, k, 16, 15), k) if normp else None
    e = P.expect_swiglu(x, w, inv)
    for name, (xm, cw, ks) in _k_mutations(x, k, sk).items():
        wm = w if cw is None else (w.double() * cw)
        mut = P.expect_swiglu(xm.double(), wm.double(), inv)
        rows = (w[:, ks] != 0).any(1)
        cols = rows[:f] | rows[f:]
        _col_tiles_hit((mut - e).abs() >= 2 * (P.REL * e.abs() + P.ABS), cols)


def test_row_side_mutations():
    m, n, k = 33, 208, 640  # row 32: the one row of the last partial x tile
    x, w, r = P.make_x(m, k, 21), P.make_w(n, k, 22), P.make_resid(m, n, 23)
    e = P.expect_plain(x, w)
    mut = e.clone()
    mut[m - 1] = e[m - 2]  # row m from row m - 1
    _row_tiles_hit((mut - e).abs() >= 1, m - 1)
    s, _ = P.expect_resid(x, w, r)
    for row in (1, m - 1):  # the residual of the neighbouring row
        rm = r.clone()
        rm[row] = r[row - 1]
        sm, _ = P.expect_resid(x, w, rm)
        _row_tiles_hit((sm.double() - s.double()).abs() >= 1, row)


@pytest.mark.parametrize("cols", [32, 64, 128])
def test_partials_from_the_unrounded_sum(cols):
    """On the integer probe rounded and unrounded sums coincide, so this mutation needs the ``frac`` residual: there
    the partials of the sum before the bf16 store leave the partials of the stored values by more than twice the
    fp32-summation allowance, in every (16 rows x one partial) tile; the stored values themselves stay exact."""
    m, n, k = 32, 256, 640
    x, w, r = P.make_x(m, k, 31), P.make_w(n, k, 32), P.make_resid(m, n, 33, frac=True)
    s, ss = P.expect_resid(x, w, r)
    unrounded = P.expect_plain(x, w) + r.double()
    assert not torch.equal(s.double(), unrounded)
    assert torch.equal(s, (unrounded.float()).to(torch.bfloat16))  # y + r is exact in fp32: one rounding either way
    good = (s.double() ** 2).view(m, -1, cols).sum(-1)
    bad = (unrounded ** 2).view(m, -1, cols).sum(-1)
    hit = (bad - good).abs() > 2 * P.part_bound(good, cols)
    assert bool(hit.view(m // MT, MT, -1).any(1).all())
    # and an fp32 sum of the stored squares, in either direction, is inside the allowance
    sq = (s.float() ** 2).view(m, -1, cols)
    for v in (sq.sum(-1), sq.flip(-1).cumsum(-1)[..., -1]):
        assert ((v.double() - good).abs() <= P.part_bound(good, cols)).all()
    assert torch.equal(ss, good.sum(1))


@pytest.mark.parametrize("p", [8, 16, 72])
@pytest.mark.parametrize("swiglu", [False, True])
def test_norm_prologue_mutations(p, swiglu):
    m, k, f = 33, 640, 48
    x = P.make_x(m, k, 41)
    w = P.make_w_swiglu(f, k, 42) if swiglu else P.make_w(2 * f, k, 42)
    part = P.make_parts(m, k, p, 43)
    inv = P.inv_of(part, k)

    def out(iv):
        return P.expect_swiglu(x, w, iv) if swiglu else P.expect_plain(x, w) * iv

    e = out(inv)
    bound = 2 * (P.REL * e.abs() + P.ABS)
    # one part_in column ignored: every row that holds mass there
    for col in (p - 1, 0, p // 2):
        pm = part.clone()
        pm[:, col] = 0
        mut = out(P.inv_of(pm, k))
        rows = (part[:, col] > 0).nonzero().flatten().tolist()
        assert rows or col != p - 1
        for row in rows:
            _row_tiles_hit((mut - e).abs() >= bound, row)
    # the inv of two neighbouring rows exchanged
    for a in (0, m - 2):
        iv = inv.clone()
        iv[[a, a + 1]] = inv[[a + 1, a]]
        mut = out(iv)
        _row_tiles_hit((mut - e).abs() >= bound, a)
        _row_tiles_hit((mut - e).abs() >= bound, a + 1)
    # the prologue left out
    mut = out(torch.ones_like(inv))
    for row in range(m):
        if abs(float(inv[row]) - 1) > 0.1:
            _row_tiles_hit((mut - e).abs() >= bound, row)


# ---- table guard -------------------------------------------------------------------------------------------------
def test_gpu_lists_are_the_ops_tables():
    """The GPU file's config lists are the op's tables (a config added later is probed by construction), and the ring
    geometry it reads from csrc/kernels/gemm_lg.hip agrees with the Python tables."""
    from chronos.ops import gemm as G

    import test_gemm_probes_gpu as T

    assert sorted(T.PP + T.LG + T.HB) == sorted(G._PP_BM) == sorted(G._PP_BN)
    assert T.HB == list(range(G.HB_FIRST, G.HB_LAST + 1))
    assert T.PP == list(range(0, G.LG_FIRST)) and not set(T.LG) & set(T.HB)
    assert T.SK == sorted(G._SK) and T.F8 == sorted(G.QLG_GEO)
    assert sorted(T.LG_GEO) == sorted(T.LG + T.HB)
    for c, (wn, xm, rb, st) in T.LG_GEO.items():
        assert (G._PP_BN[c], G._PP_BM[c]) == (wn, xm) and rb in (64, 128) and 2 <= st <= 16, c
    for c, (wn, xm, rb, st) in T.F8_GEO.items():
        assert G.QLG_GEO[c] == (xm, wn) and rb == 128, c
    assert sorted(T.F8_GEO) == T.F8
    # split-K support as the op states it
    for c in T.PP + T.LG + T.HB:
        assert T.splitk_ok(c) == G._pp_valid(c, 1024, 1024, 0, 2, 64), c
    # the routed rows name only configs of these lists
    assert T.ROUTED and {r[0] for r in T.ROUTED} <= set(T.PP + T.LG + T.HB) | {100 + c for c in T.SK}
    assert {r[0] for r in T.ROUTED_F8} <= set(T.F8)
    ids = [p.id for p in T.CASES]
    assert len(ids) == len(set(ids))
    assert {p.values[0] for p in T.CASES} == {("pp", c) for c in T.PP + T.LG + T.HB} | {("sk", c) for c in T.SK} | \
        {("f8", c) for c in T.F8}
