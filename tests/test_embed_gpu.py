"""csrc/kernels/pool.hip on the GPU: the exact ``pool_accum`` probe and the ``pool_finish`` probe of
tests/_embed_cases.py through the HIP kernels at every compiled hidden size, bit-equal repeats, and the shapes at which
the kernels take another path: one wave with two row groups (H = 256), several waves per row, ranges of one segment
(added straight into the accumulator) and of several (through the scratch rows), overlapping ranges (the segment length
doubles until the items fit), and more sequences than the plan kernel has threads."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _embed_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIDDEN = (256, 1024, 4096, 8192)


@pytest.fixture(scope="module")
def ops():
    from chronos import ops

    ops.load()
    return ops


@pytest.mark.parametrize("H", HIDDEN)
def test_pool_accum_exact_probe(ops, H):
    case = C.accum_case(H)
    C.check_accum(C.run_accum(case, DEV, ops.pool_accum), case)


@pytest.mark.parametrize("H", HIDDEN)
def test_pool_accum_same_bits_every_launch(ops, H):
    g = torch.Generator().manual_seed(H)
    s = torch.randn(700, H, generator=g).to(torch.bfloat16).to(DEV)
    q = torch.tensor([(0, 300), (300, 301), (301, 301), (310, 700)], dtype=torch.int32, device=DEV)
    sel = torch.tensor([2, 0, 1, 3], dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        acc = torch.zeros(4, H, dtype=torch.float32, device=DEV)
        ops.pool_accum(s, 1e-5, q, sel, acc)
        outs.append(acc)
    assert torch.equal(outs[0], outs[1])
    ref = torch.zeros(4, H, dtype=torch.float32)
    ops.pool_accum(s.cpu(), 1e-5, q.cpu(), sel.cpu(), ref)  # the fp64-accumulating reference
    # at most 390 fp32 additions per column, each rounding a running sum below 128 (half an ulp: 2^-18), whatever their
    # order; the terms' own error (3 * 2^-24 relative at magnitude < 8) is far below that
    assert float(ref.abs().max()) < 128
    assert float((outs[0].cpu() - ref).abs().max()) <= 390 * 2.0 ** -18
    assert float(outs[0][1].abs().max()) == 0.0


@pytest.mark.parametrize("H", (256, 4096))
def test_pool_accum_overlapping_ranges_double_the_segment(ops, H):
    """Eight sequences over the same 64 rows: 16 segments of 32 rows do not fit the 2 + 8 items sized from T and B, so
    the plan doubles the segment length for every sequence.  Exact integers again."""
    s, xn = C.probe_rows(64, H)
    q = torch.tensor([(0, 64)] * 8, dtype=torch.int32, device=DEV)
    sel = torch.tensor([7, 6, 5, 4, 3, 2, 1, 0], dtype=torch.int32, device=DEV)
    acc = torch.zeros(8, H, dtype=torch.float32, device=DEV)
    ops.pool_accum(s.to(DEV), 0.0, q, sel, acc)
    d = np.abs(acc.double().cpu().numpy() - xn.sum(0)[None, :])
    assert (d <= 64 * 2.0 ** -20).all()


def test_pool_accum_many_short_sequences(ops):
    """1500 sequences of 1-3 rows (the plan kernel's threads take several sequences each), every third one skipped."""
    H, B = 256, 1500
    lens = [1 + i % 3 for i in range(B)]
    T = sum(lens)
    s, xn = C.probe_rows(T, H)
    q, at = [], 0
    for n in lens:
        q.append((at, at + n))
        at += n
    sel = [-1 if i % 3 == 1 else i for i in range(B)]
    acc = torch.zeros(B, H, dtype=torch.float32, device=DEV)
    ops.pool_accum(s.to(DEV), 0.0, torch.tensor(q, dtype=torch.int32, device=DEV),
                   torch.tensor(sel, dtype=torch.int32, device=DEV), acc)
    e = np.zeros((B, H))
    for (lo, hi), r in zip(q, sel):
        if r >= 0:
            e[r] = xn[lo:hi].sum(0)
    assert (np.abs(acc.double().cpu().numpy() - e) <= 3 * 2.0 ** -20).all()


def test_pool_accum_refuses_other_hidden_sizes(ops):
    with pytest.raises((ValueError, RuntimeError), match="256, 1024, 4096"):
        ops.pool_accum(torch.zeros(4, 512, dtype=torch.bfloat16, device=DEV), 1e-5,
                       torch.zeros(1, 2, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                       torch.zeros(2, 512, device=DEV))


@pytest.mark.parametrize("H", HIDDEN)
def test_pool_finish_probe(ops, H):
    C.check_finish(C.finish_case(H), DEV, ops.pool_finish)
