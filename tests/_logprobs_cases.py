"""Shared cases for tests/test_logprobs.py (CPU path of ops.*) and tests/test_logprobs_gpu.py (the HIP kernels).

Expected values come from the few lines of torch in ``expected`` below (masked_fill with -inf, torch.logsumexp, a
stable sort on (-logit, id)) — never from chronos.ops.reference.

Tolerance: ids exact, logprobs 1e-3 absolute.  The inputs are exact in fp32; what differs between the code under test
and ``expected`` is the summation order of at most 131 072 positive fp32 terms (tree over 1 024 threads, about
(128 + 10) * 2^-24 ~ 1e-5 relative in the sum) and the fast exp / log intrinsics.  A forced token must give exactly 0.0.
"""
import torch

from chronos import ops

DONE = 0
TOL = 1e-3
NEG = float("-inf")
# grammar states of the synthetic DFA
ST_GEN, ST_NEAR, ST_FAR, ST_ONE, ST_FEW = 1, 2, 3, 4, 5
NSTATES = 6
FEW = 3          # legal tokens in ST_FEW
REMAINING = 10   # budget = 9: tokens leading to ST_FAR (dist 50) are removed by budget forcing
SENT_MARK, SENT_LSE, SENT_ID, SENT_VAL = 77, 123.5, -7, 55.5

KINDS = ("general", "single", "few", "neginf", "ties4", "sub_bf16", "flat")


def cases():
    """(vocab, dtype, K, kind).  1000: not a multiple of 8 and smaller than the workgroup (scalar loads); 4104: a
    multiple of 8 but not of 1024 (vector loads, ragged last iteration); 128256: one case.  9000 / 9001 (vector / scalar loads):
    more than the 8 192 tokens after which the kernel's first pass only counts tokens above a floor, and ~6 300 legal
    tokens, so a flat boundary key overflows the kernel's 4 096-entry LDS candidate list (the third pass, and for a
    single key the arg-max rounds)."""
    out = []
    for vocab in (1000, 4104):
        for dt in ("bf16", "f32"):
            for K in (1, 5, 20):
                out.append((vocab, dt, K, "general"))
            for kind in KINDS[1:]:
                if kind == "sub_bf16" and dt != "f32":
                    continue
                out.append((vocab, dt, 20 if kind in ("ties4", "sub_bf16", "flat") else 5, kind))
            out.append((vocab, dt, 5, "ties4"))
    for dt in ("bf16", "f32"):
        for kind in ("general", "ties4", "flat") + (("sub_bf16",) if dt == "f32" else ()):
            out.append((9000, dt, 20, kind))
    out.append((9001, "bf16", 5, "general"))
    out.append((9001, "f32", 20, "ties4"))
    out.append((128256, "bf16", 20, "general"))
    return out


def case_id(c):
    return f"v{c[0]}-{c[1]}-k{c[2]}-{c[3]}"


def build_dfa(vocab, g):
    """next [NSTATES, vocab] int16, dist [NSTATES] int16.  ST_GEN: ~90 % of the tokens have a transition, 20 % lead to
    ST_FAR, whose distance exceeds the budget (~70 % stay legal); ST_ONE: one legal token; ST_FEW: FEW legal tokens."""
    nxt = torch.full((NSTATES, vocab), -1, dtype=torch.int16)
    u = torch.rand(vocab, generator=g)
    nxt[ST_GEN][u < 0.9] = ST_NEAR
    nxt[ST_GEN][u < 0.2] = ST_FAR
    nxt[ST_ONE, vocab // 3] = ST_NEAR
    for t in (1, vocab // 2, vocab - 1):
        nxt[ST_FEW, t] = ST_NEAR
    nxt[ST_NEAR] = nxt[ST_GEN]
    dist = torch.tensor([0, 2, 1, 50, 2, 2], dtype=torch.int16)
    return nxt, dist


def legal_mask(nxt, dist, s, remaining):
    nx = nxt[s].long()
    return (nx >= 0) & (dist[nx.clamp(min=0)].long() <= remaining - 1)


def expected(row, legal, K):
    """(lse, top ids [K] with -1 tail, top raw logits [K] with -inf tail) of one fp32 logits row."""
    x = row.float()
    lse = torch.logsumexp(x.masked_fill(~legal, NEG), 0)
    idx = legal.nonzero().flatten()
    order = torch.sort(-x[idx], stable=True).indices[:K]  # idx ascends: equal logits stay in id order
    ids = torch.full((K,), -1, dtype=torch.int64)
    vals = torch.full((K,), NEG)
    ids[:order.numel()] = idx[order]
    vals[:order.numel()] = x[idx[order]]
    return lse, ids, vals


def make_logits(kind, vocab, dt, g):
    """Six logits rows (fp32 values exactly representable in the case's dtype) with a row stride of vocab + 8."""
    rows = 6
    if kind == "ties4":
        x = torch.tensor([-1.0, 0.0, 0.5, 2.0])[torch.randint(0, 4, (rows, vocab), generator=g)]
    elif kind == "sub_bf16":
        # all within half a bf16 ulp of 1.0: one 16-bit key, 2048 distinct fp32 values, many exact duplicates
        x = 1.0 + torch.randint(0, 2048, (rows, vocab), generator=g).float() * 2.0 ** -20
    elif kind == "flat":  # every logit equal: the whole legal set is one plateau, the answer is the K smallest ids
        x = torch.full((rows, vocab), 1.5)
    else:
        x = torch.randn(rows, vocab, generator=g) * 3.0
        x[:, ::97] = 0.0
        x[:, 5::194] = -0.0
    if kind == "neginf":
        x[torch.rand(rows, vocab, generator=g) < 0.3] = NEG
    if dt == "bf16":
        x = x.bfloat16()
    buf = torch.full((rows, vocab + 8), 9.0e3, dtype=x.dtype)  # the padding would win every arg-max if it were read
    buf[:, :vocab] = x
    return buf


class Case:
    """Six slots in one launch: 0 live, 1 DONE, 2 empty (-1), 3 parked (-2 - s), 4 row_of_slot = -1, 5 lp_want = -1."""

    def __init__(self, vocab, dt, K, kind, dev, max_out=8, seed=0):
        g = torch.Generator().manual_seed(1234 + seed)
        self.vocab, self.K, self.kind, self.dev, self.max_out = vocab, K, kind, dev, max_out
        self.nxt_c, self.dist_c = build_dfa(vocab, g)
        self.buf_c = make_logits(kind, vocab, dt, g)
        live = {"single": ST_ONE, "few": ST_FEW}.get(kind, ST_GEN)
        self.state_c = torch.tensor([live, DONE, -1, -2 - ST_GEN, ST_GEN, ST_GEN], dtype=torch.int32)
        self.row_c = torch.tensor([3, 0, 1, 2, -1, 5], dtype=torch.int32)  # slot 0 reads logits row 3
        self.nout_c = torch.tensor([3, 1, 0, 2, 4, 5], dtype=torch.int32)
        self.want_c = torch.tensor([K, K, K, K, K, -1], dtype=torch.int32)
        d = lambda t: t.to(dev)  # noqa: E731
        self.nxt, self.dist, self.buf = d(self.nxt_c), d(self.dist_c), d(self.buf_c)
        self.logits = self.buf[:, :vocab]
        self.state, self.row, self.nout, self.want = d(self.state_c), d(self.row_c), d(self.nout_c), d(self.want_c)
        self.rem = torch.full((6,), REMAINING, dtype=torch.int32, device=dev)
        self.mark = torch.full((6,), SENT_MARK, dtype=torch.int32, device=dev)
        self.lse = torch.full((6,), SENT_LSE, dtype=torch.float32, device=dev)
        self.top_ids = torch.full((6, K), SENT_ID, dtype=torch.int32, device=dev)
        self.top_val = torch.full((6, K), SENT_VAL, dtype=torch.float32, device=dev)
        self.legal = legal_mask(self.nxt_c, self.dist_c, live, REMAINING)
        self.exp = expected(self.buf_c[3, :vocab], self.legal, K)

    def pre(self):
        ops.token_logprobs(self.logits, self.row, self.nxt, self.dist, DONE, self.state, self.rem, self.nout,
                           self.want, self.mark, self.lse, self.top_ids, self.top_val)

    def ring(self):
        """Rings [6, max_out, 1 + K] / [6, max_out, K] as the middle of guarded flat buffers."""
        K, mo = self.K, self.max_out
        n1, n2, pad = 6 * mo * (1 + K), 6 * mo * K, 64
        self.flat_lp = torch.full((n1 + 2 * pad,), SENT_VAL, dtype=torch.float32, device=self.dev)
        self.flat_ids = torch.full((n2 + 2 * pad,), SENT_ID, dtype=torch.int32, device=self.dev)
        self.out_lp = self.flat_lp[pad:pad + n1].view(6, mo, 1 + K)
        self.out_ids = self.flat_ids[pad:pad + n2].view(6, mo, K)
        self.out_tok = torch.zeros(6, mo, dtype=torch.int32, device=self.dev)

    def commit(self):
        ops.token_logprobs_commit(self.logits, self.row, self.nout, self.out_tok, self.want, self.mark, self.lse,
                                  self.top_ids, self.top_val, self.out_lp, self.out_ids)

    def ring_untouched_except(self, slot=None, i=None):
        lp, ids = self.flat_lp.cpu().clone(), self.flat_ids.cpu().clone()
        if slot is not None:
            K, mo, pad = self.K, self.max_out, 64
            a = pad + (slot * mo + i) * (1 + K)
            lp[a:a + 1 + K] = SENT_VAL
            b = pad + (slot * mo + i) * K
            ids[b:b + K] = SENT_ID
        assert bool((lp == SENT_VAL).all()), "logprob ring written outside the committed entry"
        assert bool((ids == SENT_ID).all()), "id ring written outside the committed entry"


def check_pre(vocab, dt, K, kind, dev):
    c = Case(vocab, dt, K, kind, dev)
    c.pre()
    mark, lse, tid, tval = c.mark.cpu(), c.lse.cpu(), c.top_ids.cpu(), c.top_val.cpu()
    e_lse, e_ids, e_vals = c.exp
    nlegal = int(c.legal.sum())
    print(f"{case_id((vocab, dt, K, kind))}: legal {nlegal}, lse {float(lse[0]):.6f} expected {float(e_lse):.6f}, "
          f"diff {abs(float(lse[0]) - float(e_lse)):.2e}")
    # the four skipped kinds and the unwanted slot keep the sentinel pattern everywhere and get lp_mark = -1
    assert mark.tolist() == [3, -1, -1, -1, -1, -1]
    assert bool((lse[1:] == SENT_LSE).all())
    assert bool((tid[1:] == SENT_ID).all()) and bool((tval[1:] == SENT_VAL).all())
    # the live slot
    assert tid[0].tolist() == e_ids.tolist()
    assert torch.equal(tval[0], e_vals), "top values are raw logits: exact"
    assert abs(float(lse[0]) - float(e_lse)) <= TOL
    if kind == "single":
        assert nlegal == 1 and float(lse[0]) == float(e_vals[0]), "a forced token must have logprob exactly 0.0"
    if kind == "few" and K > FEW:
        assert tid[0, FEW:].tolist() == [-1] * (K - FEW) and bool((tval[0, FEW:] == NEG).all())
    if kind == "general":  # budget forcing removed otherwise legal tokens, and they are not reported
        far = (c.nxt_c[ST_GEN] == ST_FAR)
        assert int(far.sum()) > 0 and not bool(far[e_ids[e_ids >= 0]].any())
        assert not bool(far[tid[0][tid[0] >= 0].long()].any())
    if kind == "neginf":
        assert bool((c.buf_c[3, :vocab].float()[c.legal] == NEG).any())
    if kind == "ties4":  # the plateau straddles the K-th place
        v = c.buf_c[3, :vocab].float()[c.legal]
        assert int((v > e_vals[K - 1]).sum()) < K < int((v >= e_vals[K - 1]).sum())
    if kind in ("sub_bf16", "flat") and vocab == 9000:
        assert nlegal > 4096, "the plateau must overflow the kernel's LDS candidate list"
    if kind == "flat":
        assert tid[0].tolist() == c.legal.nonzero().flatten()[:K].tolist()
    if kind == "sub_bf16":
        assert len(set(c.buf_c[3, :vocab].bfloat16().tolist())) == 1 and len(set(e_vals.tolist())) > 1


def _sample_by_hand(c, tok):
    """What the sampler does to the ring inputs for slot 0: emit ``tok`` at index nout (if it fits), advance nout."""
    n = int(c.nout_c[0])
    if n < c.max_out:
        c.out_tok[0, n] = tok
    c.nout[0] = n + 1


def check_commit(vocab, dt, K, kind, dev):
    c = Case(vocab, dt, K, kind, dev)
    c.ring()
    c.pre()
    # a slot whose nout did not advance (the sampler did not run): nothing is written
    c.commit()
    c.ring_untouched_except()
    e_lse, e_ids, e_vals = c.exp
    tok = int(e_ids[min(1, K - 1)]) if int(e_ids[min(1, K - 1)]) >= 0 else int(e_ids[0])
    _sample_by_hand(c, tok)
    c.commit()
    c.ring_untouched_except(0, 3)
    lp, ids = c.out_lp[0, 3].cpu(), c.out_ids[0, 3].cpu()
    assert ids.tolist() == e_ids.tolist()
    want = torch.cat([c.buf_c[3, tok].float().reshape(1), e_vals]) - e_lse
    print(f"{case_id((vocab, dt, K, kind))}: max |logprob - expected| "
          f"{float((lp - want)[torch.isfinite(want)].abs().max()):.2e}")
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(lp), fin) and bool((lp[~fin] == NEG).all())
    assert float((lp[fin] - want[fin]).abs().max()) <= TOL
    if kind == "single":
        assert float(lp[0]) == 0.0 and float(lp[1]) == 0.0, "a forced token must have logprob exactly 0.0"


def check_commit_full_ring(vocab, dt, K, dev):
    """nout == max_out: the sampler advances nout without storing a token; the commit writes nothing."""
    c = Case(vocab, dt, K, "general", dev)
    c.ring()
    c.nout_c[0] = c.max_out
    c.nout[0] = c.max_out
    c.pre()
    assert int(c.mark[0]) == c.max_out
    _sample_by_hand(c, 0)
    c.commit()
    c.ring_untouched_except()


def check_chain(vocab, dt, K, dev):
    """token_logprobs -> constrained_sample -> commit on a greedy row: the sampled token is the first alternative."""
    c = Case(vocab, dt, K, "general", dev)
    c.ring()
    c.pre()
    i32 = dict(dtype=torch.int32, device=dev)
    ids, pos, ctx = torch.zeros(6, **i32), torch.zeros(6, **i32), torch.ones(6, **i32)
    ops.constrained_sample(c.logits, c.row, c.nxt, c.dist, DONE, c.state, c.rem, None, None, ids, pos, ctx, c.nout,
                           c.out_tok)
    assert c.nout.cpu().tolist() == [4, 1, 0, 2, 4, 6]  # slots 0 and 5 were sampled
    c.commit()
    c.ring_untouched_except(0, 3)
    tok = int(c.out_tok[0, 3])
    lp, tid = c.out_lp[0, 3].cpu(), c.out_ids[0, 3].cpu()
    assert int(tid[0]) == tok == int(c.exp[1][0])
    assert float(lp[0]) == float(lp[1])
