"""Shared cases for tests/test_mirostat.py (CPU path of ops.mirostat_truncate / ops.mirostat_update) and
tests/test_mirostat_gpu.py (the HIP kernels): Mirostat 2.0 over the sampler's legal set, csrc/kernels/mirostat.hip.

Yardstick: fp64 arithmetic written out here (``surprise``, ``oracle_mu``), not chronos.ops.reference.

EPS_S, the margin on a surprise, from the fp32 rounding of steps 1 to 3 (u = 2^-24, the relative error of one fp32
operation).  The rows used here are randn * 2 with a head raised by 8, or ladders within [-8, 8]: m - x <= 32, and
the smallest temperature is 0.5, so q = (m - x) / T <= 64.
  * m - x and the division by T: one rounding each, |dq| <= 2 u q <= 7.7e-6;
  * Z = sum exp(-q): expf is good to 2 ulp and carries dq as a relative error, <= 8e-6 per term; each thread adds at
    most 126 terms in sequence (128256 tokens / 1024 threads) and the block tree adds 10 levels, <= 136 u = 8.2e-6
    relative in the worst case; logf adds 2 ulp of ln Z <= 12, 1.5e-6: |d ln Z| <= 1.8e-5;
  * q + ln Z <= 76: one rounding, 4.6e-6;  the product with 1 / ln 2 (<= 110 bits): one rounding and the rounded
    constant, 1.4e-5 bits.
Together (7.7e-6 + 1.8e-5 + 4.6e-6) / ln 2 + 1.4e-5 = 5.8e-5 bits.  EPS_S = 2^-12 = 2.44e-4 bits is four times that
worst-case sum; it was fixed from this arithmetic before any kernel ran.

The bound on mu after one update, mu' = mu - eta * (S_obs - tau): S_obs carries the same error as S (ln Z' is a sum of
the same kind over fewer terms), scaled by eta; the subtraction, the product and the final subtraction round once each
at magnitudes below 64 (ulp 3.8e-6), together < 1.2e-5.  EPS_MU(eta) = eta * EPS_S + 2^-15 (3.05e-5).

Survivors are judged by two-sided containment: the kernel's set must contain what fp64 keeps at mu - EPS_S and nothing
fp64 removes at mu + EPS_S.  The band between the two is a property of the input and is asserted on the oracle alone:
zero in the hand-built cases, at most 1 % of the legal tokens in the random ones (mu is placed midway between two
adjacent surprise classes).  Everything outside the legal tokens of the active slots is compared bit for bit.
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _truncate_cases as tc  # noqa: E402

from chronos import ops  # noqa: E402

DONE, NEG = tc.DONE, tc.NEG
ST_GEN, ST_ONE, REMAINING = tc.ST_GEN, tc.ST_ONE, tc.REMAINING
EPS_S = 2.0 ** -12
MAX_OUT = 4
LN2 = math.log(2.0)


def eps_mu(eta):
    return eta * EPS_S + 2.0 ** -15


# ---- fp64 oracle ----------------------------------------------------------------------------------------------------
def surprise(x, legal, T, nats=False, no_T=False):
    """fp64 (S [V] with +inf outside the legal set, m, ln Z) of one row, or None for a forced step.  ``nats`` and
    ``no_T`` are the mutations "natural log for log2" and "temperature ignored"."""
    if int(legal.sum()) < 2:
        return None
    xl = x.double().masked_fill(~legal, NEG)
    m = xl.max()
    if float(m) == NEG:
        return None
    T = 1.0 if no_T else float(torch.tensor(T, dtype=torch.float32))
    q = (m - xl) / T
    lnz = torch.log(torch.exp(-q).sum())
    S = (q + lnz) / (1.0 if nats else LN2)
    return S.masked_fill(~legal, float("inf")), m, lnz


def bounds(x, legal, T, mu, eps=EPS_S, **mut):
    """(must, may) of one row, or None for a forced step.  The maxima always survive."""
    r = surprise(x, legal, T, **mut)
    if r is None:
        return None
    S, m, _ = r
    top = legal & (x.double() == m)
    return legal & ((S <= mu - eps) | top), legal & ((S <= mu + eps) | top)


def oracle_mu(x, legal, kept, tok, T, mu, tau, eta, mut=None):
    """fp64 mu after the update for token ``tok`` drawn from the survivors ``kept`` of row ``x``."""
    mut = mut or ""
    if mut == "mu_frozen":
        return mu
    if mut == "swap":
        tau, eta = eta, tau
    T = 1.0 if mut == "no_T" else float(torch.tensor(T, dtype=torch.float32))
    xl = x.double()
    m = xl.masked_fill(~legal, NEG).max()
    q = (m - xl) / T
    z = torch.exp(-q)[legal if mut == "z_for_zprime" else kept].sum()
    sobs = float((q[tok] + torch.log(z)) / (1.0 if mut == "nats" else LN2))
    return mu - eta * (sobs - tau)


def midway_mu(x, legal, T, frac):
    """A mu (exact in fp32) midway between two adjacent surprise classes of the row, about ``frac`` of the way up the
    sorted legal surprises."""
    S = surprise(x, legal, T)[0]
    cls = torch.unique(S[legal & (S < float("inf"))])
    j = min(max(int(frac * cls.numel()), 0), cls.numel() - 2)
    return float(torch.tensor((float(cls[j]) + float(cls[j + 1])) / 2, dtype=torch.float32))


# ---- slots ----------------------------------------------------------------------------------------------------------
def slot(kind="live", x=None, state=ST_GEN, T=1.0, on=1, mu=10.0, tau=5.0, eta=0.1, nout=1, band0=False):
    """One slot of a case.  kind: live | done | parked | empty | norow.  ``x`` None = a NaN-filled row."""
    return dict(kind=kind, x=x, state=state, T=T, on=on, mu=mu, tau=tau, eta=eta, nout=nout, band0=band0)


class Case:
    """Slots over len(slots) + 1 logits rows of width vocab + 8 (poison in the padding), permuted through row_of_slot
    (``rows="perm"``) or identity without it (``rows=None``)."""

    def __init__(self, name, vocab, dt, nxt, dist, slots, rows="perm"):
        self.name, self.vocab, self.dt, self.nxt, self.dist, self.slots, self.rows = name, vocab, dt, nxt, dist, slots, rows
        n = self.n = len(slots)
        dtype = torch.bfloat16 if dt == "bf16" else torch.float32
        self.perm = list(range(n, 0, -1)) if rows == "perm" else list(range(n))
        buf = torch.full((n + 1, vocab + 8), tc.POISON, dtype=dtype)
        for s, sp in enumerate(slots):
            buf[self.perm[s], :vocab] = float("nan") if sp["x"] is None else sp["x"].to(dtype)
        self.buf = buf
        st = {"done": DONE, "empty": -1}
        self.state = torch.tensor([st.get(sp["kind"], -2 - sp["state"] if sp["kind"] == "parked" else sp["state"])
                                   for sp in slots], dtype=torch.int32)
        self.row = torch.tensor([-1 if sp["kind"] == "norow" else self.perm[s] for s, sp in enumerate(slots)],
                                dtype=torch.int32)
        f32 = lambda k: torch.tensor([float(sp[k]) for sp in slots], dtype=torch.float32)  # noqa: E731
        self.temp, self.mu, self.tau, self.eta = f32("T"), f32("mu"), f32("tau"), f32("eta")
        self.on = torch.tensor([sp["on"] for sp in slots], dtype=torch.int32)
        self.nout = torch.tensor([sp["nout"] for sp in slots], dtype=torch.int32)
        self.rem = torch.full((n,), REMAINING, dtype=torch.int32)

    def legal(self, s):
        return tc.legal_mask(self.nxt, self.dist, self.slots[s]["state"], REMAINING)

    def x(self, s):
        """The row of slot s as the kernel reads it (rounded to the buffer's dtype), fp32."""
        return self.buf[self.perm[s], :self.vocab].float()

    def sampled(self, s):
        """Does the sampler emit a token for slot s?"""
        return self.slots[s]["kind"] == "live"

    def active(self, s):
        """Does mirostat truncate slot s (and move its mu)?  Live, on, sampling, and not a forced step."""
        sp = self.slots[s]
        return sp["kind"] == "live" and bool(sp["on"]) and sp["T"] > 0 and surprise(self.x(s), self.legal(s), sp["T"]) \
            is not None

    def check_input(self):
        """The band between the two containment sets, on the oracle alone."""
        for s, sp in enumerate(self.slots):
            if not self.active(s):
                continue
            must, may = bounds(self.x(s), self.legal(s), sp["T"], float(self.mu[s]))
            band, nl = int((may & ~must).sum()), int(self.legal(s).sum())
            assert band == 0 if sp["band0"] else band <= 0.01 * nl, (self.name, s, band, nl)

    def run(self, dev, sample=True, truncate=None, update=None):
        """mirostat_truncate, constrained_sample (``sample``), mirostat_update on ``dev``; everything back on the host.
        ``truncate`` / ``update`` replace the ops (the mutation tests pass fp64 impostors)."""
        d = lambda t: t.clone().to(dev)  # noqa: E731
        buf = d(self.buf)
        logits = buf[:, :self.vocab] if self.rows == "perm" else buf[:self.n, :self.vocab]
        row = d(self.row) if self.rows == "perm" else None
        nxt, dist, state, rem, nout, temp = d(self.nxt), d(self.dist), d(self.state), d(self.rem), d(self.nout), d(self.temp)
        on, mu, tau, eta = d(self.on), d(self.mu), d(self.tau), d(self.eta)
        n = self.n
        m, lnz = torch.full((n,), 77.0, device=dev), torch.full((n,), 77.0, device=dev)
        mark = torch.full((n,), 3, dtype=torch.int32, device=dev)  # stale marks: every launch must rewrite them
        out = torch.full((n, MAX_OUT), -1, dtype=torch.int32, device=dev)
        (truncate or ops.mirostat_truncate)(logits, row, nxt, dist, DONE, state, rem, nout, temp, on, mu, m, lnz, mark)
        res = dict(buf=buf.cpu().clone(), mark=mark.cpu().clone(), m=m.cpu().clone(), lnz=lnz.cpu().clone(),
                   mu0=mu.cpu().clone())
        if sample:
            i32 = dict(dtype=torch.int32, device=dev)
            ids, pos, ctx = (torch.zeros(n, **i32) for _ in range(3))
            ops.constrained_sample(logits, row, nxt, dist, DONE, state, rem, temp, torch.arange(n, **i32) + 5, ids, pos,
                                   ctx, nout, out, torch.zeros(n, **i32), torch.ones(n, device=dev))
        (update or ops.mirostat_update)(logits, row, nout, out, temp, on, mu, tau, eta, m, lnz, mark)
        res.update(buf2=buf.cpu(), nout=nout.cpu(), out=out.cpu(), mu=mu.cpu(), mark2=mark.cpu(), m2=m.cpu(),
                   lnz2=lnz.cpu())
        return res

    def violations(self, res, scale=1.0, sample=True):
        """What in ``res`` lies outside the bounds (margins times ``scale``): a list of strings, empty = all good."""
        bad = []
        want = self.buf.clone()
        mask = torch.zeros_like(want, dtype=torch.bool)
        for s, sp in enumerate(self.slots):
            tag = f"{self.name} slot {s}"
            if not self.active(s):
                if int(res["mark"][s]) != -1:
                    bad.append(f"{tag}: mark {int(res['mark'][s])} on a slot mirostat must leave alone")
                if res["mu"][s].view(torch.int32) != self.mu[s].view(torch.int32):
                    bad.append(f"{tag}: mu moved on a slot mirostat must leave alone: {float(res['mu'][s])}")
                continue
            x, legal, T, mu0 = self.x(s), self.legal(s), sp["T"], float(self.mu[s])
            mask[self.perm[s], :self.vocab] = legal
            got = res["buf"][self.perm[s], :self.vocab].float()
            kept = legal & (got > NEG)
            must, may = bounds(x, legal, T, mu0, EPS_S * scale)
            if bool((must & ~kept).any()):
                bad.append(f"{tag}: {int((must & ~kept).sum())} tokens fp64 keeps with margin were removed")
            if bool((kept & ~may).any()):
                bad.append(f"{tag}: {int((kept & ~may).sum())} tokens fp64 removes with margin were kept")
            if not torch.equal(got[kept], x[kept]):
                bad.append(f"{tag}: a survivor's logit was rewritten")
            if set(x[kept].tolist()) & set(x[legal & ~kept & (x > NEG)].tolist()):
                bad.append(f"{tag}: equal logits did not share their fate")
            if int(res["mark"][s]) != sp["nout"]:
                bad.append(f"{tag}: mark {int(res['mark'][s])}, not nout {sp['nout']}")
            if float(res["m"][s]) != float(x[legal].max()):
                bad.append(f"{tag}: m {float(res['m'][s])}")
            if not bool(kept.any()):
                continue
            zp = float(torch.log(torch.exp((x.double()[kept] - float(x[legal].max())) /
                                           float(torch.tensor(T, dtype=torch.float32))).sum()))
            if abs(float(res["lnz"][s]) - zp) > EPS_S * LN2 * scale:
                bad.append(f"{tag}: ln Z' {float(res['lnz'][s])} against {zp}")
            if not sample:
                if res["mu"][s].view(torch.int32) != self.mu[s].view(torch.int32):
                    bad.append(f"{tag}: mu moved although the sampler emitted nothing")
                continue
            tok = int(res["out"][s, sp["nout"]]) if sp["nout"] < MAX_OUT else -1
            if not (0 <= tok < self.vocab and bool(kept[tok])):
                bad.append(f"{tag}: the sampler drew token {tok}, not a survivor")
                continue
            mu1 = oracle_mu(x, legal, kept, tok, T, mu0, sp["tau"], sp["eta"])
            if not abs(float(res["mu"][s]) - mu1) <= eps_mu(sp["eta"]) * scale:
                bad.append(f"{tag}: mu {float(res['mu'][s])} against {mu1} (bound {eps_mu(sp['eta']) * scale})")
        if not tc.same_bits(res["buf"].masked_fill(mask, 0), want.masked_fill(mask, 0)):
            bad.append(f"{self.name}: something outside the active slots' legal tokens moved")
        if not tc.same_bits(res["buf2"], res["buf"]):
            bad.append(f"{self.name}: the update kernel wrote to the logits")
        for k in ("mark", "m", "lnz"):
            if not torch.equal(res[k], res[k + "2"]):
                bad.append(f"{self.name}: the update kernel wrote to {k}")
        return bad

    def report(self, res):
        for s, sp in enumerate(self.slots):
            if self.active(s):
                kept = self.legal(s) & (res["buf"][self.perm[s], :self.vocab].float() > NEG)
                print(f"{self.name} slot {s}: T {sp['T']} mu {float(self.mu[s]):.5f} -> {float(res['mu'][s]):.5f} "
                      f"kept {int(kept.sum())} of {int(self.legal(s).sum())}")


# ---- the cases ------------------------------------------------------------------------------------------------------
def random_case(vocab, dt, T, rows, seed):
    """Three random rows (live), each at its own midway mu, plus a parked NaN row."""
    g = torch.Generator().manual_seed(300 + seed)
    nxt, dist = tc.build_dfa(vocab, g)
    legal = tc.legal_mask(nxt, dist, ST_GEN, REMAINING)
    x = tc.random_rows(vocab, dt, g, n=3)
    x[:, (~legal).nonzero().flatten()[:1]] = 60.0  # an illegal token holds the largest logit of every row
    x[0, legal.nonzero().flatten()[-3:]] = NEG     # legal -inf logits stay what they are
    if dt == "bf16":
        x = x.bfloat16().float()
    sl = [slot(x=x[i], T=T, mu=midway_mu(x[i], legal, T, f), tau=tau, eta=eta, nout=i)
          for i, (f, tau, eta) in enumerate(((0.02, 5.0, 0.1), (0.3, 3.0, 0.25), (0.7, 8.0, 1.0)))]
    sl.insert(1, slot("parked"))
    return Case(f"random v{vocab} {dt} T{T} {rows}", vocab, dt, nxt, dist, sl, rows)


def ladder_case(vocab, dt, rows="perm", seed=0):
    """Hand-built rows (ladders: surprise classes 0.5 / T / ln 2 bits apart, band zero) and every kind of slot:
    0 live, mu cuts the ladder in the middle      1 DONE (NaN row)        2 parked (NaN row)     3 empty (NaN row)
    4 no row (row_of_slot -1; identity: live)      5 greedy, temperature 0  6 mirostat off         7 mu so low that only
    the maxima survive, two tokens tied at the top 8 mu so high that nothing is removed             9 one legal token
    10 every legal logit -inf                      11 live at T 2, eta > tau                        12 live, nout at the
    last output index."""
    g = torch.Generator().manual_seed(400 + seed)
    nxt, dist = tc.build_dfa(vocab, g)
    legal = tc.legal_mask(nxt, dist, ST_GEN, REMAINING)
    lad = [tc.ladder_row(vocab, legal, g) for _ in range(4)]
    tie = lad[1].clone()
    tie[(tie == 7.5).nonzero().flatten()] = 8.0  # the second rung joins the first: a tie at the maximum
    assert int((tie[legal] == 8.0).sum()) == 2
    ninf = lad[2].clone()
    ninf[legal] = NEG
    mid = lambda x, T, j: float(torch.tensor(float(surprise(x, legal, T)[0][legal].unique()[j:j + 2].mean()),  # noqa: E731
                                             dtype=torch.float32))
    norow = "norow" if rows == "perm" else "live"
    sl = [slot(x=lad[0], T=0.5, mu=mid(lad[0], 0.5, 6), band0=True, nout=0),
          slot("done"), slot("parked"), slot("empty"),
          slot(norow, x=lad[3], T=1.0, mu=mid(lad[3], 1.0, 3), band0=True),
          slot(x=lad[0], T=0.0, mu=1.0),
          slot(x=lad[0], T=1.0, on=0, mu=1.0),
          slot(x=tie, T=1.0, mu=-3.0, tau=0.5, eta=0.3, band0=True),
          slot(x=lad[1], T=1.0, mu=1.0e3, tau=2.0, eta=0.5, band0=True, nout=2),
          slot(x=lad[2], state=ST_ONE, mu=0.5),
          slot(x=ninf, mu=0.5),
          slot(x=lad[3], T=2.0, mu=mid(lad[3], 2.0, 9), tau=0.25, eta=1.5, band0=True),
          slot(x=lad[2], T=1.0, mu=mid(lad[2], 1.0, 2), band0=True, nout=MAX_OUT - 1)]
    return Case(f"ladder v{vocab} {dt} {rows}", vocab, dt, nxt, dist, sl, rows)


def check(case, dev, sample=True):
    case.check_input()
    res = case.run(dev, sample=sample)
    case.report(res)
    bad = case.violations(res, sample=sample)
    assert not bad, "\n".join(bad)
    return res


def check_all(dev, big=True):
    """The whole module on ``dev``: what tests/test_mirostat.py runs on the reference and test_mirostat_gpu.py on the
    kernels."""
    for dt in ("bf16", "f32"):
        for rows in ("perm", None):
            check(ladder_case(1003, dt, rows), dev)
        check(ladder_case(5003, dt), dev)
        for i, T in enumerate((0.5, 1.0, 2.0)):
            check(random_case(5003, dt, T, "perm" if i % 2 else None, seed=i), dev)
            check(random_case(1003, dt, T, None if i % 2 else "perm", seed=10 + i), dev)
    if big:
        check(random_case(128256, "bf16", 1.0, "perm", seed=20), dev)
        check(random_case(128256, "f32", 0.5, None, seed=21), dev)
    check(ladder_case(1003, "bf16"), dev, sample=False)  # nout does not advance: no mu moves


# ---- mutations: fp64 impostors of the two ops -----------------------------------------------------------------------
MUTATIONS = ("mu_frozen", "z_for_zprime", "nats", "no_T", "forced_moves", "swap")


def impostor(case, mut):
    """(truncate, update) with the ops' signatures, computing in fp64 on the host what the kernels should (``mut``
    None) or a wrong variant of it."""
    tmut = dict(nats=mut == "nats", no_T=mut == "no_T")
    kept_of = {}

    def truncate(logits, row, nxt, dist, done, state, rem, nout, temp, on, mu, m, lnz, mark):
        for s in range(case.n):
            mark[s] = -1
            if not case.active(s):
                continue
            r = case.perm[s]
            x, legal = case.x(s), case.legal(s)
            S = surprise(x, legal, float(temp[s]), **tmut)[0]
            kept = legal & ((S <= float(mu[s])) | (x == x[legal].max()))
            logits[r, (legal & ~kept & (x > NEG)).nonzero().flatten()] = NEG
            kept_of[s] = kept
            mark[s], m[s] = int(nout[s]), x[legal].max()
            lnz[s] = float(torch.log(torch.exp((x.double()[kept] - float(m[s])) / float(temp[s])).sum()))

    def update(logits, row, nout, out, temp, on, mu, tau, eta, m, lnz, mark):
        for s in range(case.n):
            sp = case.slots[s]
            if mut == "forced_moves" and case.sampled(s) and sp["on"] and sp["T"] > 0 and not case.active(s):
                mu[s] = float(mu[s]) - float(eta[s]) * (0.0 - float(tau[s]))  # llama.cpp books surprise 0
            if int(mark[s]) < 0 or int(nout[s]) != int(mark[s]) + 1:
                continue
            tok = int(out[s, int(mark[s])])
            mu[s] = oracle_mu(case.x(s), case.legal(s), kept_of[s], tok, float(temp[s]), float(mu[s]), float(tau[s]),
                              float(eta[s]), mut)

    return truncate, update
