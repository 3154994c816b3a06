"""Shared cases for tests/test_truncate.py (CPU path of ops.truncate_logits) and tests/test_truncate_gpu.py (the HIP
kernel): min_p / typical_p, llama.cpp's semantics on raw logits over the sampler's legal set.

Yardsticks.  min_p is one fp32 comparison ``x >= m' + ln p`` on exact inputs, so a written row must equal the
reference's bit for bit.  typical_p is judged against fp64 arithmetic written out here (``typical_stats``), not
against chronos.ops.reference:

* constructed rows (a ladder of distinct logits over a floor) with the boundary placed so that the accumulated mass
  misses ``tp`` by >= 1e-3 on both sides and the neighbouring classes are >= 1e-2 away in ``d``: the fp32 kernel
  cannot legitimately decide differently (its error in ``d`` is <= 5e-5, in mass far below 1e-4), so the survivor
  set must be exactly the fp64 one;
* random rows: two-sided containment with margins EPS_M = 1e-4 on mass and EPS_D = 1e-3 on ``d`` (about 20x the
  fp32-vs-fp64 error), and the undecided band between the two sets may hold at most 10 % of the fp64 survivors.
"""
import math

import torch

from chronos import ops

DONE = 0
NEG = float("-inf")
POISON = 9.0e3
EPS_M, EPS_D = 1e-4, 1e-3
ST_GEN, ST_NEAR, ST_FAR, ST_ONE = 1, 2, 3, 4
REMAINING = 10  # budget 9: tokens that lead to ST_FAR (dist 50) are illegal by budget forcing


def build_dfa(vocab, g):
    """next [5, vocab] int16, dist [5] int16: in ST_GEN ~90 % of the tokens have a transition, 20 % lead to ST_FAR
    (too far for the budget), so ~70 % are legal; ST_ONE has one legal token."""
    nxt = torch.full((5, vocab), -1, dtype=torch.int16)
    u = torch.rand(vocab, generator=g)
    nxt[ST_GEN][u < 0.9] = ST_NEAR
    nxt[ST_GEN][u < 0.2] = ST_FAR
    nxt[ST_NEAR] = nxt[ST_GEN]
    nxt[ST_ONE, vocab // 3] = ST_NEAR
    return nxt, torch.tensor([0, 2, 1, 50, 2], dtype=torch.int16)


def legal_mask(nxt, dist, s, remaining):
    nx = nxt[s].long()
    return (nx >= 0) & (dist[nx.clamp(min=0)].long() <= remaining - 1)


def typical_stats(x, legal):
    """fp64 (p, d) of the legal tokens of one row (illegal ones: p = 0, d = +inf)."""
    xl = x.double().masked_fill(~legal, NEG)
    logp = xl - torch.logsumexp(xl, 0)
    p = torch.exp(logp)
    H = -torch.where(p > 0, p * logp, torch.zeros_like(p)).sum()
    d = (-logp - H).abs().masked_fill(~legal, float("inf"))
    return p, d


def typical_boundary(p, d, tp):
    """(d*, mass strictly below the boundary class, mass including it, d of the class before, d of the class after)."""
    order = torch.sort(d, stable=True).indices
    ds, cum = d[order], torch.cumsum(p[order], 0)
    over = (cum > tp).nonzero().flatten()
    i = int(over[0]) if over.numel() else ds.numel() - 1
    dstar = ds[i]
    lo, hi = ds < dstar, ds <= dstar
    below = float(cum[lo][-1]) if bool(lo.any()) else 0.0
    upto = float(cum[hi][-1])
    prev = float(ds[lo][-1]) if bool(lo.any()) else -math.inf
    nxt = float(ds[~hi][0]) if bool((~hi).any()) else math.inf
    return float(dstar), below, upto, prev, nxt


def typical_keep(x, legal, tp):
    p, d = typical_stats(x, legal)
    return legal & (d <= typical_boundary(p, d, tp)[0])


def typical_bounds(x, legal, tp):
    """(must, may, R): the kernel's set must contain ``must`` (what fp64 keeps at tp - EPS_M, less the tokens within
    EPS_D below that boundary) and lie inside ``may`` (what fp64 keeps at tp + EPS_M, widened by EPS_D)."""
    p, d = typical_stats(x, legal)
    lo = typical_boundary(p, d, tp - EPS_M)[0]
    hi = typical_boundary(p, d, tp + EPS_M)[0]
    return legal & (d <= lo - EPS_D), legal & (d <= hi + EPS_D), legal & (d <= typical_boundary(p, d, tp)[0])


def ladder_row(vocab, legal, g, steps=20, top=8.0, step=0.5, floor=-8.0):
    """fp32 row (values exact in bf16): ``steps`` legal tokens on a ladder top, top - step, ... (geometric in
    probability), every other legal token on the floor, illegal tokens at random values up to 40 (one of them the
    largest logit of the row)."""
    x = torch.full((vocab,), floor)
    idx = legal.nonzero().flatten()
    pick = idx[torch.randperm(idx.numel(), generator=g)[:steps]]
    x[pick] = top - step * torch.arange(steps, dtype=torch.float32)
    ill = (~legal).nonzero().flatten()
    x[ill] = torch.randint(-40, 41, (ill.numel(),), generator=g).float()
    x[ill[0]] = 64.0
    return x


def ladder_tp(x, legal, j):
    """A typical_p whose boundary is the j-th class by ascending d, midway in mass, with the margins asserted."""
    p, d = typical_stats(x, legal)
    order = torch.sort(d, stable=True).indices
    ds, cum = d[order], torch.cumsum(p[order], 0)
    cls = torch.unique_consecutive(ds)
    upto = float(cum[ds <= cls[j]][-1])
    below = float(cum[ds < cls[j]][-1]) if j else 0.0
    tp = float(torch.tensor((below + upto) / 2, dtype=torch.float32))
    dstar, b, u, prev, nxt = typical_boundary(p, d, tp)
    assert dstar == float(cls[j])
    assert tp - b >= 1e-3 and u - tp >= 1e-3, ("mass margin", tp - b, u - tp)
    assert dstar - prev >= 1e-2 and nxt - dstar >= 1e-2, ("gap in d", dstar - prev, nxt - dstar)
    return tp


class Slots:
    """``n`` slots over ``n + 1`` logits rows of width vocab + 8 (poison in the padding), rows permuted through
    row_of_slot (``rows="perm"``) or identity without it (``rows=None``).  With n >= 3 some slots are DONE, parked,
    empty, unsampled (row -1), greedy (temperature 0) or neutral: ``kinds[slot]``."""

    KINDS = ("live", "done", "parked", "empty", "norow", "greedy", "neutral", "live")

    def __init__(self, n, vocab, dt, dev, nxt, dist, live_state, x_rows, minp, typ, rows="perm", remaining=REMAINING):
        self.n, self.vocab, self.dev = n, vocab, dev
        if n >= 8:
            self.kinds = [self.KINDS[i % 8] for i in range(n)]
        elif n == 3:
            self.kinds = ["live", "parked", "live"]
        else:
            self.kinds = ["live"] * n
        dtype = torch.bfloat16 if dt == "bf16" else torch.float32
        buf = torch.full((n + 1, vocab + 8), POISON, dtype=dtype)
        perm = list(range(n, 0, -1)) if rows == "perm" else list(range(n))
        for slot in range(n):
            buf[perm[slot], :vocab] = x_rows[slot % len(x_rows)].to(dtype)
        st = {"live": live_state, "done": DONE, "parked": -2 - live_state, "empty": -1}
        self.state_c = torch.tensor([st.get(k, live_state) for k in self.kinds], dtype=torch.int32)
        self.row_c = torch.tensor([-1 if k == "norow" else perm[s] for s, k in enumerate(self.kinds)],
                                  dtype=torch.int32)
        self.temp_c = torch.tensor([0.0 if k == "greedy" else 0.8 for k in self.kinds])
        self.minp_c = torch.tensor([NEG if k == "neutral" else (math.log(minp[s % len(minp)]) if minp[s % len(minp)]
                                                                 else NEG) for s, k in enumerate(self.kinds)])
        self.typ_c = torch.tensor([1.0 if k == "neutral" else typ[s % len(typ)] for s, k in enumerate(self.kinds)])
        self.rem_c = torch.full((n,), remaining, dtype=torch.int32)
        self.perm, self.rows = perm, rows
        self.nxt_c, self.dist_c, self.buf_c, self.live_state, self.remaining = nxt, dist, buf, live_state, remaining
        self.legal = legal_mask(nxt, dist, live_state, remaining)

    def run(self):
        """ops.truncate_logits on self.dev; returns the whole written buffer on the host."""
        d = lambda t: t.to(self.dev)  # noqa: E731
        buf = d(self.buf_c.clone())
        logits = buf[:, :self.vocab] if self.rows == "perm" else buf[:self.n, :self.vocab]
        ops.truncate_logits(logits, d(self.row_c) if self.rows == "perm" else None, d(self.nxt_c), d(self.dist_c), DONE,
                            d(self.state_c), d(self.rem_c), d(self.temp_c), d(self.minp_c), d(self.typ_c))
        return buf.cpu()

    def active(self):
        """Slots the kernel must rewrite (everything else must stay bit for bit)."""
        return [s for s, k in enumerate(self.kinds) if k == "live"]

    def expected(self, keep_of_slot):
        """The buffer with -inf in the legal non-survivors of every active slot; keep_of_slot(slot, row) -> mask."""
        out = self.buf_c.clone()
        for s in self.active():
            r = self.perm[s]
            keep = keep_of_slot(s, self.buf_c[r, :self.vocab].float())
            assert bool(keep.any()) and not bool((keep & ~self.legal).any())
            out[r, :self.vocab][self.legal & ~keep] = NEG
        return out

    def survivors(self, buf, slot):
        """What survived in the written buffer: legal tokens of the slot's row that are not -inf."""
        return self.legal & (buf[self.perm[slot], :self.vocab].float() > NEG)


def same_bits(a, b):
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return torch.equal(a.view(it), b.view(it))


def random_rows(vocab, dt, g, n=3):
    """randn * 2; in bf16 ten logits of each row raised by 8 (a peaked head over a wide tail)."""
    x = torch.randn(n, vocab, generator=g) * 2.0
    if dt == "bf16":
        for r in range(n):
            x[r, torch.randperm(vocab, generator=g)[:10]] += 8.0
        x = x.bfloat16().float()
    return x


def check_minp(n, vocab, dt, dev, nxt=None, dist=None, live_state=ST_GEN, rows="perm", seed=0, remaining=REMAINING):
    g = torch.Generator().manual_seed(100 + seed)
    if nxt is None:
        nxt, dist = build_dfa(vocab, g)
    x = random_rows(vocab, dt, g, n=min(n, 4))
    legal = legal_mask(nxt, dist, live_state, remaining)
    x[:, (~legal).nonzero().flatten()[:1]] = 60.0  # an illegal token holds the largest logit of every row
    x[0, legal.nonzero().flatten()[-3:]] = NEG     # legal -inf logits stay what they are
    c = Slots(n, vocab, dt, dev, nxt, dist, live_state, list(x), minp=(0.05, 1.0, 1e-4), typ=(1.0,), rows=rows,
              remaining=remaining)
    got = c.run()
    want = c.expected(lambda s, row: ops.truncate_survivors(row, c.legal, float(c.minp_c[s]), 1.0))
    for s in c.active():  # the reference mask is the formula itself
        row = c.buf_c[c.perm[s], :vocab].float()
        m = row[c.legal].max()
        assert torch.equal(c.survivors(want, s), c.legal & (row >= m + c.minp_c[s]) & (row > NEG))
    assert any(int(c.survivors(want, s).sum()) < int(c.legal.sum()) for s in c.active())
    assert same_bits(got, want), "min_p: the written buffer differs from the reference's"
    return c, got


def check_typical_ladder(vocab, dt, dev, with_minp, seed=0):
    g = torch.Generator().manual_seed(200 + seed)
    nxt, dist = build_dfa(vocab, g)
    legal = legal_mask(nxt, dist, ST_GEN, REMAINING)
    rows = [ladder_row(vocab, legal, g) for _ in range(3)]
    tps = [ladder_tp(rows[s], legal, j) for s, j in enumerate((1, 0, 8))]
    minp = (0.3,) if with_minp else (0.0,)
    c = Slots(3, vocab, dt, dev, nxt, dist, ST_GEN, rows, minp=minp, typ=tps)
    assert c.kinds == ["live", "parked", "live"]

    def keep(s, row):
        k = typical_keep(row, legal, tps[s])
        if with_minp:
            k &= row >= row[k].max() + c.minp_c[s]
        r32 = ops.truncate_survivors(row, legal, float(c.minp_c[s]), tps[s])
        assert torch.equal(k, r32) and torch.equal(k, ops.truncate_survivors(row, legal, float(c.minp_c[s]), tps[s],
                                                                             torch.float64))
        return k

    want = c.expected(keep)
    got = c.run()
    for s in c.active():
        a, b = c.survivors(got, s), c.survivors(want, s)
        print(f"ladder v{vocab} {dt} slot {s}: tp {tps[s]:.6f} survivors {int(a.sum())} expected {int(b.sum())}")
        assert torch.equal(a, b), "typical_p: the survivor set differs from the fp64 one"
    assert same_bits(got, want)
    # in slot 0 typical_p removes the most probable token, so min_p keys off the maximum of what is left
    assert not bool(typical_keep(rows[0], legal, tps[0])[rows[0].masked_fill(~legal, NEG).argmax()])


def check_typical_random(dt, dev, tp, seed, vocab=128256):
    g = torch.Generator().manual_seed(seed)
    nxt, dist = build_dfa(vocab, g)
    legal = legal_mask(nxt, dist, ST_GEN, REMAINING)
    rows = list(random_rows(vocab, dt, g, n=3))
    bounds = [typical_bounds(r, legal, tp) for r in rows]
    for must, may, R in bounds:  # a condition on the input, checked before the kernel runs
        band = int((may & ~must).sum())
        assert band <= 0.10 * int(R.sum()), ("undecided band too wide for this input", band, int(R.sum()))
    c = Slots(3, vocab, dt, dev, nxt, dist, ST_GEN, rows, minp=(0.0,), typ=(tp,))
    got = c.run()
    for s in c.active():
        must, may, R = bounds[s]
        k = c.survivors(got, s)
        row = rows[s]
        print(f"random {dt} tp {tp} seed {seed} slot {s}: kept {int(k.sum())} fp64 {int(R.sum())} "
              f"must {int(must.sum())} may {int(may.sum())}")
        assert bool(k.any())
        assert not bool((must & ~k).any()), "a token fp64 keeps with margin was removed"
        assert not bool((k & ~may).any()), "a token fp64 removes with margin was kept"
        kept_vals, dropped_vals = set(row[k].tolist()), set(row[legal & ~k].tolist())
        assert not (kept_vals & dropped_vals), "equal logits must share their fate"
    untouched = c.buf_c.clone()
    mask = torch.zeros_like(untouched, dtype=torch.bool)
    for s in c.active():
        mask[c.perm[s], :vocab] = legal
    assert same_bits(got.masked_fill(mask, 0), untouched.masked_fill(mask, 0)), "something outside the legal set moved"


def check_sampler_after(dev, vocab=1003):
    """constrained_sample on truncated rows (64 slots, temperature 1, with and without top_k = 4) returns a survivor."""
    g = torch.Generator().manual_seed(7)
    nxt, dist = build_dfa(vocab, g)
    legal = legal_mask(nxt, dist, ST_GEN, REMAINING)
    n = 64
    x = (torch.randn(n, vocab, generator=g) * 2.0).bfloat16()
    d = lambda t: t.to(dev)  # noqa: E731
    i32 = dict(dtype=torch.int32, device=dev)
    lnp = torch.full((n,), math.log(0.2))
    keep = [ops.truncate_survivors(x[s].float(), legal, float(lnp[s]), 1.0) for s in range(n)]
    assert all(1 <= int(k.sum()) < int(legal.sum()) for k in keep) and any(int(k.sum()) > 4 for k in keep)
    for topk in (0, 4):
        logits = d(x.clone())
        state, rem = torch.full((n,), ST_GEN, **i32), torch.full((n,), REMAINING, **i32)
        temp, seed = torch.ones(n, device=dev), torch.arange(n, **i32)
        ops.truncate_logits(logits, None, d(nxt), d(dist), DONE, state, rem, temp, d(lnp), torch.ones(n, device=dev))
        ids, pos, ctx, nout = (torch.zeros(n, **i32) for _ in range(4))
        out = torch.zeros(n, 4, **i32)
        ops.constrained_sample(logits, None, d(nxt), d(dist), DONE, state, rem, temp, seed, ids, pos, ctx, nout, out,
                               torch.full((n,), topk, **i32), torch.ones(n, device=dev))
        assert nout.cpu().tolist() == [1] * n
        chosen = out[:, 0].cpu().tolist()
        assert all(bool(keep[s][chosen[s]]) for s in range(n)), "the sampler drew a truncated token"
        assert len(set(chosen)) > 1
