"""Shared engine-level Mirostat 2.0 checks for tests/test_mirostat.py (CPU) and tests/test_mirostat_engine_gpu.py.

Two ways to see what the engine did, both judged with the fp64 oracle and the margins of tests/_mirostat_cases.py:

* ``Recorder`` wraps ``ops.mirostat_truncate`` / ``ops.mirostat_update`` and clones, at every (eager) launch, the
  logits row, the legal set and mu of every mirostat slot before the launch, and the emitted token and mu after the
  update.  One step is then checked on its own (token among the survivors, mu within EPS_MU of the oracle's), and the
  steps must chain bit for bit: nothing but the update kernel moves mu — not a forced step, not a jumped run, not a
  preemption.
* the public surface: ``logprobs = 20`` on a grammar whose states have at most 20 legal tokens returns the whole legal
  distribution of every step (x - lse: the surprise is invariant under the shift), and ``Request.mirostat_mu``, read
  at every harvest of a one-step burst through the streaming callback, is mu after each token.  (Runs of the same
  request with num_predict = 1..n would not do: budget forcing narrows the legal set of a short run's last tokens,
  so they are not prefixes of the long run.)  The logprobs carry
  the fp32 rounding of x - lse (|x|, |lse| < 32: 2 ulp = 7.6e-6, at most 2.2e-5 bits at T = 0.5), which widens the
  margin on S to EPS_S + 2^-15 here.

A token inside the undecided band makes Z' two-valued; the bound on mu is then the hull of both (``step_bounds``).
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mirostat_cases as mc  # noqa: E402
import _truncate_cases as tc  # noqa: E402
from _truncate_engine import prompts, run  # noqa: E402,F401

from chronos import ops  # noqa: E402
from chronos.brain.engine.engine import Engine, EngineConfig  # noqa: E402
from chronos.sensor.prompt import VERDICT_SCHEMA  # noqa: E402

# ten items out of seven words: every grammar state has at most 17 legal tokens (asserted where it is used)
WORDS = {"type": "array", "minItems": 10, "maxItems": 10,
         "items": {"type": "string", "enum": ["red", "green", "blue", "cyan", "pink", "grey", "gold"]}}
EPS_LP = 2.0 ** -15


def engine(dev, **kw):
    base = dict(model="tiny", device=dev, max_slots=8, max_model_len=384, use_graphs=False, decode_burst=4,
                jump_forward=True, max_logprobs=20, penalty_window=64)
    base.update(kw)
    return Engine(EngineConfig(**base))


def mi(**kw):
    return dict(dict(temperature=1.0, seed=11, mirostat=2, mirostat_tau=1.5, mirostat_eta=0.5), **kw)


def step_bounds(x, tok, T, mu0, tau, eta, eps=mc.EPS_S):
    """x: fp32 logits of the legal tokens of one step (>= 2 of them, not all -inf).  Returns (tok may survive, lo, hi):
    is ``tok`` inside the widened fp64 survivor set, and the hull of the oracle's mu after the update."""
    legal = torch.ones_like(x, dtype=torch.bool)
    must, may = mc.bounds(x, legal, T, mu0, eps)
    mus = [mc.oracle_mu(x, legal, k | (torch.arange(x.numel()) == tok), tok, T, mu0, tau, eta) for k in (must, may)]
    return bool(may[tok]), min(mus) - mc.eps_mu(eta) - eta * (eps - mc.EPS_S), max(mus) + mc.eps_mu(eta) + \
        eta * (eps - mc.EPS_S)


class Recorder:
    """[dict(rid, i, x, legal, T, mu0, tok, mu1)] per mirostat slot and launch, in launch order."""

    def __init__(self, eng, monkeypatch):
        self.eng, self.steps, self._open = eng, [], []
        real_t, real_u = ops.mirostat_truncate, ops.mirostat_update

        def truncate(logits, row_of_slot, next_tab, dist, done_state, state, remaining, nout, temp, on, mu, *a):
            owner = {r.slot: r for r in (*eng.prefilling, *eng.running.values())}
            rows = row_of_slot.cpu().tolist() if row_of_slot is not None else list(range(state.numel()))
            self._open = []
            for slot, s in enumerate(state.cpu().tolist()):
                r = owner.get(slot)
                if s <= 0 or rows[slot] < 0 or r is None or not r.mirostat:
                    continue
                assert int(on[slot]) == 1
                legal = tc.legal_mask(next_tab.cpu(), dist.cpu(), s, int(remaining[slot]))
                self._open.append(dict(rid=r.rid, i=len(r.resume_out) + int(nout[slot]), slot=slot, n0=int(nout[slot]),
                                       x=logits[rows[slot], :next_tab.shape[1]].float().cpu().clone(), legal=legal,
                                       T=float(temp[slot]), mu0=mu[slot].cpu().clone()))
            real_t(logits, row_of_slot, next_tab, dist, done_state, state, remaining, nout, temp, on, mu, *a)
            for st in self._open:
                st["row"] = logits[rows[st["slot"]], :next_tab.shape[1]].float().cpu().clone()

        def update(logits, row_of_slot, nout, out, temp, on, mu, *a):
            real_u(logits, row_of_slot, nout, out, temp, on, mu, *a)
            for st in self._open:
                assert int(nout[st["slot"]]) == st["n0"] + 1, "the sampler did not advance a live mirostat slot"
                st["tok"], st["mu1"] = int(out[st["slot"], st["n0"]]), mu[st["slot"]].cpu().clone()
                self.steps.append(st)
            self._open = []

        monkeypatch.setattr(ops, "mirostat_truncate", truncate)
        monkeypatch.setattr(ops, "mirostat_update", update)

    def of(self, r):
        return [st for st in self.steps if st["rid"] == r.rid]


def bits(t):
    return int(torch.as_tensor(t, dtype=torch.float32).view(torch.int32))


def check_steps(rec, r, mu_start=None):
    """Every recorded step of request r on its own, and the chain from ``mu_start`` (default 2 * tau) to
    ``r.mirostat_mu`` bit for bit.  Returns (free steps, forced steps, steps that removed a token)."""
    steps = rec.of(r)
    assert steps, "mirostat never ran for the request"
    mu = 2.0 * r.mirostat_tau if mu_start is None else mu_start
    free = forced = cut = 0
    for st in steps:
        assert bits(st["mu0"]) == bits(mu), (r.rid, st["i"], "mu moved between two sampler launches", float(st["mu0"]), mu)
        x, legal = st["x"], st["legal"]
        if st["i"] < len(r.out_ids):  # (the step that drew the stop token is not part of out_ids)
            assert r.out_ids[st["i"]] == st["tok"]
        if int(legal.sum()) < 2 or float(x[legal].max()) == tc.NEG:
            assert bits(st["mu1"]) == bits(st["mu0"]), (r.rid, st["i"], "a forced step moved mu")
            assert torch.equal(st["row"][legal], x[legal])
            forced += 1
        else:
            idx = legal.nonzero().flatten()
            ok, lo, hi = step_bounds(x[idx], int((idx == st["tok"]).nonzero()), st["T"], float(st["mu0"]),
                                     r.mirostat_tau, r.mirostat_eta)
            assert ok, (r.rid, st["i"], st["tok"], "the emitted token is not a survivor")
            assert lo <= float(st["mu1"]) <= hi, (r.rid, st["i"], float(st["mu1"]), lo, hi)
            assert torch.equal(st["row"][~legal], x[~legal])
            free += 1
            cut += int((st["row"][legal] > tc.NEG).sum()) < int((x[legal] > tc.NEG).sum())
        mu = float(st["mu1"])
    assert bits(r.mirostat_mu) == bits(mu), (r.rid, "Request.mirostat_mu is not mu after the last sampled token",
                                             r.mirostat_mu, mu)
    return free, forced, cut


# ---- trajectory through the public surface --------------------------------------------------------------------------
def check_trajectory(dev, **cfg):
    """One-step bursts: the streaming callback sees Request.mirostat_mu after every token; the whole legal distribution
    of every step comes back as logprobs.  Steps 1 to 5 replayed on the host from those alone."""
    eng = engine(dev, decode_burst=1, small_burst=1, jump_forward=False, **cfg)
    seen = []
    r = eng.submit(prompts(1)[0], fmt=WORDS, num_predict=60, logprobs=20,
                   meta={"on_tokens": lambda toks: seen.append((len(toks), r.mirostat_mu))}, **mi(temperature=0.7))
    eng.run_until_idle()
    n = len(r.out_ids)  # (num_predict leaves the grammar room: budget forcing would make forced steps of free ones)
    assert r.done_reason == "stop" and r.mirostat and n >= 30 and len(r.out_logprobs) == n
    mus, k = {0: 2.0 * r.mirostat_tau}, 0
    for cnt, mu in seen:
        k += cnt
        mus[k] = mu
    # (the token sampled by the prefill step is harvested together with the first burst's: mu after it is not seen)
    assert k == n + 1 and len(mus) >= n and bits(mus[k]) == bits(r.mirostat_mu)  # (n tokens and the stop token)
    free = moved = 0
    a = b = mus[0]  # the hull of mu before step i: a point wherever the engine showed it
    for i, (lp, top) in enumerate(r.out_logprobs):
        ids, x = [t for t, _ in top], torch.tensor([v for _, v in top], dtype=torch.float32)
        assert len(ids) <= 17 and abs(float(torch.exp(x.double()).sum()) - 1.0) < 1e-4, "not the whole legal set"
        if len(ids) >= 2:
            tok = ids.index(r.out_ids[i])
            ends = [step_bounds(x, tok, r.temperature, mu0, r.mirostat_tau, r.mirostat_eta, eps=mc.EPS_S + EPS_LP)
                    for mu0 in (a, b)]
            assert ends[1][0], (i, r.out_ids[i], "the emitted token is not a survivor")
            a, b = min(e[1] for e in ends), max(e[2] for e in ends)
            free += 1
        if i + 1 in mus:
            print(f"step {i}: {len(ids)} legal, mu -> {mus[i + 1]:.6f} in [{a:.6f}, {b:.6f}]")
            assert a <= mus[i + 1] <= b, (i, mus[i + 1], a, b)
            if i in mus:
                if len(ids) < 2:
                    assert bits(mus[i + 1]) == bits(mus[i]), (i, "a forced token moved mu")
                else:
                    moved += bits(mus[i + 1]) != bits(mus[i])
            a = b = mus[i + 1]
    assert free >= n // 2 and moved >= free - 2
    return eng, r


# ---- jump-forward ---------------------------------------------------------------------------------------------------
def check_jump_forward(dev, monkeypatch, **cfg):
    """A verdict-schema request with jump-forward on: forced runs appended by the host and forced single tokens leave
    mu alone; the final mu is the chain of the sampled steps only."""
    eng = engine(dev, max_logprobs=0, **cfg)
    rec = Recorder(eng, monkeypatch)
    r, = run(eng, [(prompts(1)[0], mi(fmt=VERDICT_SCHEMA, num_predict=60, seed=5))])
    assert r.meta.get("jump_spans"), "the request never jumped"
    free, forced, cut = check_steps(rec, r)
    jumped = sum(k for _, k in r.meta["jump_spans"])
    total = len(r.out_ids) + (r.done_reason == "stop")
    print(f"jump-forward: {free} free, {forced} forced, {jumped} jumped of {total} tokens; {cut} steps cut; "
          f"mu {r.mirostat_mu:.5f}")
    assert free > 0 and cut > 0 and free + forced + jumped >= len(r.out_ids)
    assert eng.stats["mirostat_launches"] > 0
    return eng, r


# ---- preemption -----------------------------------------------------------------------------------------------------
def check_preemption(dev, monkeypatch, **cfg):
    """A request preempted after a few tokens is re-admitted with the mu it had, not 2 * tau."""
    eng = engine(dev, decode_burst=2, small_burst=2, max_logprobs=0, **cfg)
    rec = Recorder(eng, monkeypatch)
    r = eng.submit(prompts(1)[0], fmt=WORDS, num_predict=30, **mi())
    while len(rec.of(r)) < 6:
        eng.step()
    assert eng.running.get(r.slot) is r
    eng._preempt(r)
    saved = r.mirostat_mu
    assert r.preemptions == 1 and bits(saved) == bits(rec.of(r)[-1]["mu1"]) and bits(saved) != bits(2 * r.mirostat_tau)
    n0 = len(rec.of(r))
    eng.run_until_idle()
    assert r.done_reason in ("stop", "length") and len(rec.of(r)) > n0
    assert bits(rec.of(r)[n0]["mu0"]) == bits(saved), "the re-admitted request did not resume from its saved mu"
    check_steps(rec, r)
    return eng, r


# ---- slot reuse, off path, mixed batches ----------------------------------------------------------------------------
def check_slot_reuse(dev, monkeypatch):
    """One slot, three requests in turn: mirostat, plain, mirostat again.  The plain one runs with the flag off, the
    third starts from its own 2 * tau."""
    p = prompts(3)
    eng = engine(dev, max_slots=1)
    rec = Recorder(eng, monkeypatch)
    first = eng.submit(p[0], fmt=WORDS, num_predict=40, **mi())
    eng.run_until_idle()
    launches = eng.stats["mirostat_launches"]
    assert first.mirostat and launches > 0 and bits(first.mirostat_mu) != bits(2 * first.mirostat_tau)
    second = eng.submit(p[1], fmt=WORDS, num_predict=40, temperature=1.0, seed=11)
    eng.run_until_idle()
    assert not second.mirostat and eng.stats["mirostat_launches"] == launches
    assert int(eng.s_mion[0]) == 0
    third = eng.submit(p[2], fmt=WORDS, num_predict=40, **mi(mirostat_tau=3.0))
    while not eng.running:
        eng.step()  # (the prefill step initialises the slot and samples the first token)
    assert int(eng.s_mion[0]) == 1 and float(eng.s_mitau[0]) == 3.0
    eng.run_until_idle()
    assert third.mirostat and bits(rec.of(third)[0]["mu0"]) == bits(6.0) and not rec.of(second)
    check_steps(rec, third)
    return eng


def plain_subs():
    p = prompts(4, seed=9)
    return [(p[0], dict(fmt=VERDICT_SCHEMA, num_predict=30, temperature=1.0, seed=3, top_k=4, top_p=0.9)),
            (p[1], dict(fmt=VERDICT_SCHEMA, num_predict=30)),
            (p[2], dict(fmt=None, num_predict=10)),
            (p[3], dict(fmt=None, num_predict=12, temperature=0.8, seed=2, min_p=0.1))]


def check_never_asked(dev, **cfg):
    """Nobody asks (or asks at temperature 0, or for version 1): no tensors, no launches, the parent's graph keys."""
    eng = engine(dev, **cfg)
    subs = plain_subs()
    subs.append((subs[1][0], dict(fmt=None, num_predict=8, mirostat=2, mirostat_tau=1.0)))  # greedy: neutral
    subs.append((subs[1][0], dict(fmt=None, num_predict=8, temperature=0.9, seed=1, mirostat=1)))  # version 1: off
    reqs = run(eng, subs)
    assert not any(r.mirostat for r in reqs)
    assert eng.stats["mirostat_launches"] == 0
    assert all(getattr(eng, a) is None for a in ("s_mion", "s_mimu", "s_mitau", "s_mieta", "s_mim", "s_milnz",
                                                 "s_mimark", "_snap_mu"))
    assert all("mi" not in k for k in eng._graphs)
    assert all(len(k) == 3 or (len(k) == 4 and k[3] == 1) or (len(k) == 5 and k[4] == "pen")
               or (len(k) == 6 and k[5] == "tr") for k in eng._graphs)
    return eng, reqs


def check_mixed(dev, **cfg):
    """A mirostat request next to sampled, greedy and truncating ones: their tokens equal a run without it."""
    subs = plain_subs()
    extra = (prompts(1, seed=13)[0], mi(fmt=WORDS, num_predict=30, top_k=3, top_p=0.5, min_p=0.4))
    eng = engine(dev, **cfg)
    on = run(eng, subs + [extra])
    m = on[-1]
    assert m.mirostat and not m.truncates and (m.top_k, m.top_p, m.min_p, m.typical_p) == (0, 1.0, 0.0, 1.0)
    assert eng.stats["mirostat_launches"] > 0
    off_eng = engine(dev, **cfg)
    off = run(off_eng, subs + [(extra[0], dict(fmt=WORDS, num_predict=30))])
    assert off_eng.stats["mirostat_launches"] == 0 and off_eng.s_mion is None
    for a, b in zip(on[:-1], off[:-1]):
        assert a.out_ids == b.out_ids and a.text == b.text and a.done_reason == b.done_reason
        assert not a.mirostat
    return eng, on


def graph_subs():
    p = prompts(3, seed=21)
    return [(p[0], mi(fmt=WORDS, num_predict=40)),
            (p[1], mi(fmt=None, num_predict=24, seed=2, mirostat_tau=4.0, mirostat_eta=0.2)),
            (p[2], mi(fmt=VERDICT_SCHEMA, num_predict=60, seed=5))]


def check_graph_equals_eager(dev, **cfg):
    """k-step graph bursts against the same engine with graphs off: the same tokens, the same final mu bit for bit."""
    out = []
    for graphs in (True, False):
        eng = engine(dev, use_graphs=graphs, max_logprobs=0, **cfg)
        reqs = run(eng, graph_subs())
        assert eng.stats["mirostat_launches"] > 0 and all(r.mirostat for r in reqs)
        if graphs:
            assert any(k[-1] == "mi" for k in eng._graphs), list(eng._graphs)
        out.append(reqs)
    for a, b in zip(*out):
        assert a.out_ids == b.out_ids and a.done_reason == b.done_reason
        assert bits(a.mirostat_mu) == bits(b.mirostat_mu), (a.mirostat_mu, b.mirostat_mu)
        assert bits(a.mirostat_mu) != bits(2 * a.mirostat_tau)
    return out
