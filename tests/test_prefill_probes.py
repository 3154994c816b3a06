"""CPU side of the prefill-attention probes (tests/_prefill_probes.py): the builders, the poison placement, the causal
lengths and the closed forms are proven against the project's fp32 reference attention; the comb's needles are shown to
sit on every edge the kernels have; and five mutations of the reference's inputs show that the probes, under the GPU
tolerance, notice a dropped key, a key read past the context, two exchanged V columns, two exchanged K rows (the pair
``kperm`` swaps) and a block table shifted by one entry — for every shape tests/test_prefill_probes_gpu.py launches."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prefill_probes as pp  # noqa: E402

CASES = [(s, k, f) for s, (_, kinds) in pp.SHAPES.items() for k in kinds for f in (False, True)]
IDS = [f"{s}-{k}-{'fp8' if f else 'bf16'}" for s, k, f in CASES]
C_SHAPES = [s for s, (_, kinds) in pp.SHAPES.items() if "C" in kinds]


def test_hadamard_rows_are_orthogonal():
    H = pp.hadamard()
    assert torch.equal(H.abs(), torch.ones(128, 128)) and bool((H[:, 0] == 1).all())
    assert torch.equal(H @ H.T, 128.0 * torch.eye(128))
    # the needle score of the docstring: a b 128 / sqrt(128) nat = 65.3 log2 units
    assert abs(pp.A_Q * pp.B_K * 128 / 128 ** 0.5 * pp.LOG2E - 65.3) < 0.05


def test_code_rows_cover_the_probe_contexts():
    n = pp.MAX_CTX + 5 * 8 + 1
    c = pp.code_rows(n)
    assert torch.unique(c, dim=0).shape[0] == n
    assert torch.equal((c / pp.V_SCALE).to(torch.float8_e4m3fn).float() * pp.V_SCALE, c)
    for L in (1, 129, 1133, pp.MAX_CTX):
        assert int(pp.u_counts(L, 7).max()) <= 18


@pytest.mark.parametrize("shape,kind,fp8", CASES, ids=IDS)
def test_reference_matches_closed_form(shape, kind, fp8):
    p = pp.probe(shape, kind, fp8)
    out = pp.reference(p)
    assert float((out - p.expect).abs().max()) <= 1e-5
    assert not bool(pp.violations(out, p).any())
    ks, vs = p.scales
    assert ks != vs or not fp8  # the two cache scales differ: a kernel that mixes them up shows
    for t, s in ((p.k, ks), (p.v, vs)):  # finite values only, poison included
        assert bool(torch.isfinite(pp._load(t, fp8, s)).all())
    # poison: the padding block, and every slot at or past ctx of a last page
    K, V = pp._load(p.k, fp8, ks), pp._load(p.v, fp8, vs)
    assert bool((K[p.pad, :, :, 0] == pp.POISON_K0).all()) and bool((V[p.pad] == pp.POISON_V).all())
    for b, c in enumerate(p.ctx.tolist()):
        if c % p.bs:
            blk = int(p.bt[b, c // p.bs])
            assert bool((K[blk, :, c % p.bs:, 0] == pp.POISON_K0).all())
            assert bool((V[blk, :, :, c % p.bs:] == pp.POISON_V).all())
        assert bool((p.bt[b, (c + p.bs - 1) // p.bs:] == p.pad).all())
    if kind == "U":
        assert bool((p.q[..., 0] > 0).all())  # every row scores a poison key high
    else:
        assert pp.margin_log2(p) >= 55.0  # and every key outside the class scores exactly 0 (asserted inside)
        n = (torch.tensor(p.lens)[:, None] - p.t0 + 127) // 128
        assert 1 <= int(n.min()) and int(n.max()) <= 9


def _both(p, a, b, seq):
    return bool(pp.holds(p, a, seq).any()) and bool(pp.holds(p, b, seq).any())


@pytest.mark.parametrize("shape", C_SHAPES)
def test_comb_needles_cover_the_edges(shape):
    kw = pp.SHAPES[shape][0]
    p = pp.probe(shape, "C")
    Lt = torch.tensor(p.lens)[:, None]
    seqs = range(p.B)
    assert bool(pp.holds(p, 0).any())  # the first key
    diag = (Lt - 1 - p.t0) % 128 == 0
    masked = ((Lt - p.t0) % 128 == 0) & (Lt > 128)  # s = -1: the class of the first masked key
    assert bool(diag.any()) and bool(masked.any())
    assert bool((p.sdist[masked] == -1).any())
    # both sides of a 32-key step edge that is no 64-key edge, of a 64-key edge and of a page edge, in one sequence
    assert any(_both(p, e - 1, e, b) for b in seqs for e in range(32, int(p.ctx[b]), 64))
    assert any(_both(p, e - 1, e, b) for b in seqs for e in range(64, int(p.ctx[b]), 64))
    assert any(_both(p, e - 1, e, b) for b in seqs for e in range(p.bs, int(p.ctx[b]), p.bs))
    # both sides of the boundary between the cached prefix and the chunk, in every sequence that has a prefix and at
    # least 64 rows (enough for the sweep to reach the two positions)
    for b, pre in enumerate(p.prefix):
        if pre and p.q_lens[b] * p.hq >= 64:
            assert _both(p, pre - 1, pre, b), b
    assert any(pre and _both(p, pre - 1, pre, b) for b, pre in enumerate(p.prefix))
    for b, c in enumerate(p.ctx.tolist()):
        if c > 1025:  # the long sequence: the 1024-token window
            assert all(bool(pp.holds(p, x, b).any()) for x in (1023, 1024, 1025))
    if kw.get("splits"):  # the last key of one kv split and the first of the next, in one 32-row tile's sequence
        G = p.hq // p.hkv
        tpw = max(1, 32 // G)
        for ns in pp.NSPLITS:
            found = False
            for b, n in enumerate(p.q_lens):
                for r0 in range(0, n, tpw):
                    kv_end = p.prefix[b] + min(n, r0 + tpw)
                    chunk = ((kv_end + ns - 1) // ns + 31) & ~31
                    rows = slice(int(p.qs[b]) + r0, int(p.qs[b]) + min(n, r0 + tpw))
                    for e in range(chunk, kv_end, chunk):
                        found |= bool(pp.holds(p, e - 1)[rows].any()) and bool(pp.holds(p, e)[rows].any())
            assert found, ns
    # rows: the diagonal needle and the first-masked-key needle sit in every one of a tile's four waves, and a needle
    # of each sort in a last, partial tile
    w = pp.waves(p)
    tpw8 = 128 // (p.hq // p.hkv)
    deep = (Lt > 128).expand(-1, p.hq)  # rows that have a masked key of a class they can see
    for wave in range(4):
        assert bool(diag[w == wave].any()), wave
        assert bool(masked[w == wave].any()) or not bool(deep[w == wave].any()), wave
    assert sum(bool(masked[w == wave].any()) for wave in range(4)) >= 2
    partial = torch.cat([torch.arange(n) >= n // tpw8 * tpw8 for n in p.q_lens])[:, None].expand(-1, p.hq)
    assert bool(diag[partial].any()) and bool(masked[partial].any())


@pytest.mark.parametrize("shape,kind,fp8", CASES, ids=IDS)
def test_mutations_are_noticed(shape, kind, fp8):
    """The probes have teeth: each mutation of the reference's inputs lands outside the GPU tolerance — by a factor of
    at least 2 in every row it must move — and, where the mutation's reach is known exactly, nowhere else."""
    p = pp.probe(shape, kind, fp8)
    seq_of = torch.tensor(p.seq_of)
    for name, mutate in pp.MUTATIONS.items():
        kw, ok, must, exact = mutate(p)
        assert any(ok), name
        ex = pp.excess(pp.reference(p, **kw), p)
        if kind == "U" and name == "swap_k":  # K = 0 everywhere: not U's to notice
            assert not bool(must.any()) and not bool((ex > 1).any())
            continue
        if kind == "U" and name == "swap_v":  # a uniform average sees only the row that splits the pair
            assert torch.equal(ex > 1, must)
            continue
        for b, o in enumerate(ok):  # flagged in every sequence the mutation applies to
            assert not o or bool(must[seq_of == b].any()), (name, b)
        assert float(ex[must].min()) >= 2.0, (name, float(ex[must].min()))
        if exact:
            assert torch.equal(ex > 1, must), name
