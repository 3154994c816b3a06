"""CPU side of the decode-attention probes (tests/_decode_probes.py): the builders, the poison placement, the causal
lengths and the closed forms are proven against the project's fp32 reference attention, and three mutations of the
reference's inputs show that the probes, under the GPU tolerance, notice a dropped key, two swapped V columns and a
block-table window shifted by one block — for every shape tests/test_decode_probes_gpu.py launches."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _decode_probes as dp  # noqa: E402

CASES = [(s, k, f) for s, (_, fp8_ok) in dp.SHAPES.items() for k in dp.shape_kinds(s)
         for f in ((False, True) if fp8_ok else (False,))]
IDS = [f"{s}-{k}-{'fp8' if f else 'bf16'}" for s, k, f in CASES]


def test_code_rows_are_unique_and_exact():
    n = 4096 + 5 * 8 + 1  # every t + 5 h a probe can ask for
    c = dp.code_rows(n)
    assert torch.unique(c, dim=0).shape[0] == n
    assert bool((c.abs() <= 7.5).all()) and torch.equal(c * 2, (c * 2).round())  # half-integers
    assert torch.equal(c.to(torch.bfloat16).float(), c)
    assert torch.equal((c / dp.KV_SCALE).to(torch.float8_e4m3fn).float() * dp.KV_SCALE, c)
    # neighbours (what a swapped or shifted key returns) differ by >= 0.5 in most dims
    assert int(((c[1:] - c[:-1]).abs() >= 0.5).sum(-1).min()) > 64


def test_u_counts_are_integer_arithmetic():
    for L in (1, 2, 127, 128, 129, 1025, 4096):
        for h in (0, 3, 7):
            want = torch.zeros(128, dtype=torch.int64)
            for t in range(L):
                want[(t + 5 * h) % 128] += 1
            assert torch.equal(dp.u_counts(L, h), want)
            assert int(want.max()) <= 32


@pytest.mark.parametrize("shape,kind,fp8", CASES, ids=IDS)
def test_reference_matches_closed_form(shape, kind, fp8):
    p = dp.probe(shape, kind, fp8)
    out = dp.reference(p)
    assert float((out - p.expect).abs().max()) <= 1e-6
    assert not bool(dp.violations(out, p).any())
    # finite values only, poison included
    for t in (p.k, p.v, p.k_pre, p.v_pre):
        if t is not None:
            assert bool(torch.isfinite(dp._load(t, fp8)).all())
    if kind != "U":
        assert dp.margin_log2(p) >= 30.0  # leak below L * 2^-30: the expectation is exact


@pytest.mark.parametrize("shape", list(dp.SHAPES))
def test_needles_cover_the_edges(shape):
    kw = dp.SHAPES[shape][0]
    cov = dp.coverage(dp.probe(shape, "N"))
    assert cov["first"] and cov["last"]
    if max(kw["ctx"]) >= 64 and kw["hq"] >= 16:
        assert cov["step_edge"]  # a 32-token step edge - 1, + 0, + 1
    if max(kw["ctx"]) >= 64 and kw["hq"] >= 32:
        assert cov["step_slots"]  # every slot 0..31 of one 32-token step
    if max(kw["ctx"]) > 1025 and kw["hq"] >= 32 and "q_lens" not in kw and not kw.get("splits"):
        assert cov["window"]  # 1023, 1024, 1025: the 64-entry block-table window
    if kw.get("splits"):
        for ns in (2, 3, 4, 16):  # the last key of one split and the first key of the next, in one sequence
            assert any({e - 1, e} <= held for c, held in zip(kw["ctx"], cov["per_seq"])
                       for e in range(((c + ns - 1) // ns + 31) & ~31, c, ((c + ns - 1) // ns + 31) & ~31)), ns
    if kw.get("prefix"):
        P = kw["prefix"]
        both = cov["positions"] | dp.coverage(dp.probe(shape, "N1"))["positions"]
        assert {0, 16 * P - 1, 16 * P, 16 * P + 1} <= both  # inside the prefix, its last key, just past it
    if "rope" in kw:  # needles at the new token and at older positions
        p = dp.probe(shape, "N")
        new = p.needle == (p.ctx.long() - 1)[:, None]
        assert bool(new.any()) and bool((~new).any())


def _seq_rows(p, seqs):
    qs = p.qs.tolist()
    return [r for b in seqs for r in range(qs[b], qs[b + 1])]


@pytest.mark.parametrize("shape,kind,fp8", CASES, ids=IDS)
def test_mutations_are_noticed(shape, kind, fp8):
    """The probes have teeth: each mutation of the reference's inputs lands outside the GPU tolerance."""
    p = dp.probe(shape, kind, fp8)
    # drop the last valid key.  U: every row of every mutated sequence moves (count - 1 over L - 1 against count over
    # L).  N: exactly the heads whose needle was that key lose it.
    kw, ok = dp.mutate_drop_last(p)
    bad = dp.violations(dp.reference(p, **kw), p)
    rows = _seq_rows(p, [b for b, o in enumerate(ok) if o])
    assert rows
    if kind == "U":
        assert bool(bad[rows].all())
    else:
        lens = torch.tensor(p.lens)
        hit = (p.needle == lens[:, None] - 1)[rows]
        assert bool(hit.any()) and torch.equal(bad[rows], hit)
    # shift the block-table window by one block.  U: every row counts other positions and a poison block.  N: K and V
    # move together, so what shows is the key that fell off the front (needles in the first block) and the poison
    # block at the end, which is a needle for the sequence's first MFMA column (its first token's first head per kv
    # head; not under RoPE, where that block's K is rotated for another sequence's position).
    kw, _ = dp.mutate_shift_window(p)
    bad = dp.violations(dp.reference(p, **kw), p)
    if kind == "U":
        assert bool(bad.all())
    else:
        G = p.hq // p.hkv
        must = p.needle < dp.BS
        if p.qkv is None:
            must[p.qs[:-1].long(), ::G] = True
        assert bool(must.any()) and bool(bad[must].all())
    # swap two V columns within one step.  A uniform average cannot see a permutation of V, so this is N's to notice:
    # the head whose needle's V moved returns the neighbour's code row.
    kw, ok = dp.mutate_swap_v(p)
    bad = dp.violations(dp.reference(p, **kw), p)
    if kind == "U":
        assert not bool(bad[torch.tensor(p.lens) >= 2].any())
    else:
        firsts = [int(p.qs[b]) for b, o in enumerate(ok) if o]
        assert firsts and bool(bad[firsts, 0].all())
