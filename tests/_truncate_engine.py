"""Shared engine-level min_p / typical_p checks for tests/test_truncate.py (CPU) and tests/test_truncate_engine_gpu.py.

A recorder wraps ``ops.truncate_logits`` and clones, at every (eager) call, the logits row of every slot whose request
truncates — before and after the launch — with its grammar state and remaining budget.  What the engine did is then
judged on those recorded rows with the yardsticks of tests/_truncate_cases.py: a min_p row bit for bit against the
reference mask, the token a ``min_p = 1`` request emitted against the maximum legal logit of its row, the token a
typical_p request emitted against the fp64 set widened by EPS_M / EPS_D."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _truncate_cases as tc  # noqa: E402

from chronos import ops  # noqa: E402
from chronos.brain.engine.engine import Engine, EngineConfig  # noqa: E402
from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt  # noqa: E402
from chronos.sensor.replay import synthetic_chains  # noqa: E402

TR_KEYS = ("min_p", "typical_p")


def engine(dev, **kw):
    base = dict(model="tiny", device=dev, max_slots=8, max_model_len=384, use_graphs=False, decode_burst=4,
                jump_forward=True, max_logprobs=5, penalty_window=64)
    base.update(kw)
    return Engine(EngineConfig(**base))


def prompts(n, seed=4):
    return [build_prompt(c.history) for c in synthetic_chains(n, seed=seed, native=False)]


def run(eng, subs):
    reqs = [eng.submit(p, **kw) for p, kw in subs]
    eng.run_until_idle()
    for r in reqs:
        assert r.done_reason in ("stop", "length"), (r.done_reason, r.error)
    return reqs


def without_truncation(subs):
    return [(p, {k: v for k, v in kw.items() if k not in TR_KEYS}) for p, kw in subs]


class Recorder:
    """{(request id, output index): (row before, row after, grammar state, remaining)} of every truncation launch."""

    def __init__(self, eng, monkeypatch):
        self.eng, self.rec = eng, {}
        real = ops.truncate_logits

        def wrapped(logits, row_of_slot, next_tab, dist, done_state, state, remaining, *a, **k):
            keys = self.note(logits, row_of_slot, state, remaining)
            real(logits, row_of_slot, next_tab, dist, done_state, state, remaining, *a, **k)
            for key, row in keys:
                self.rec[key] += (logits[row, :next_tab.shape[1]].float().cpu().clone(),)

        monkeypatch.setattr(ops, "truncate_logits", wrapped)

    def note(self, logits, row_of_slot, state, remaining):
        eng = self.eng
        owner = {r.slot: r for r in (*eng.prefilling, *eng.running.values())}
        st, rem, no = state.cpu().tolist(), remaining.cpu().tolist(), eng.s_nout.cpu().tolist()
        rows = row_of_slot.cpu().tolist() if row_of_slot is not None else list(range(len(st)))
        V = eng.bank.next.shape[1]
        keys = []
        for slot, s in enumerate(st):
            r = owner.get(slot)
            if s <= 0 or rows[slot] < 0 or r is None or not r.truncates:
                continue
            key = (r.rid, len(r.resume_out) + no[slot])
            assert key not in self.rec, "an output index was truncated twice"
            self.rec[key] = (logits[rows[slot], :V].float().cpu().clone(), s, rem[slot])
            keys.append((key, rows[slot]))
        return keys

    def steps(self, r):
        """[(output index, row before, row after, legal mask)] of request r, by output index."""
        nxt, dist = self.eng.bank.next.cpu(), self.eng.bank.dist.cpu()
        out = []
        for (rid, i), (pre, s, rem, post) in sorted(self.rec.items(), key=lambda kv: kv[0]):
            if rid == r.rid:
                out.append((i, pre, post, tc.legal_mask(nxt, dist, s, rem)))
        return out


def check_minp_request(rec, r, minp):
    """Every recorded step of a min_p-only request: the row the sampler saw is the reference's bit for bit, and the
    emitted token survived.  With min_p = 1 its logit equals the maximum legal logit of the step's row."""
    steps = rec.steps(r)
    assert steps, "the request was never truncated"
    free = 0
    for i, pre, post, legal in steps:
        keep = ops.truncate_survivors(pre, legal, math.log(minp), 1.0)
        want = pre.clone()
        want[legal & ~keep] = tc.NEG
        assert tc.same_bits(post, want), (r.rid, i)
        if i >= len(r.out_ids):  # the step that drew the stop token, which is not part of out_ids
            continue
        tok = r.out_ids[i]
        assert bool(keep[tok]), (r.rid, i, tok)
        if minp == 1.0:
            assert float(pre[tok]) == float(pre[legal].max()), (r.rid, i, tok, float(pre[tok]), float(pre[legal].max()))
        free += int(legal.sum()) > 1
    assert free, "every recorded step was grammar-forced: the check saw no choice"
    return len(steps)


def check_typical_request(rec, r, tp, minp=0.0):
    """Every token a typical_p request emitted lies in the fp64 set widened by the margins (and, with a min_p, not
    below the widened set's own min_p cut)."""
    steps = rec.steps(r)
    assert steps
    removed = 0
    for i, pre, post, legal in steps:
        if i >= len(r.out_ids):  # the step that drew the stop token, which is not part of out_ids
            continue
        tok = r.out_ids[i]
        assert post[tok] == pre[tok] and float(post[tok]) > tc.NEG, (r.rid, i, tok)
        if int(legal.sum()) < 2:
            assert tc.same_bits(post, pre)
            continue
        must, may, R = tc.typical_bounds(pre, legal, tp)
        assert bool(may[tok]), (r.rid, i, tok)
        kept = legal & (post > tc.NEG)
        assert not bool((kept & ~may).any()) and bool(kept.any())
        if not minp:
            assert not bool((must & ~kept).any())
        removed += int((legal & ~kept & (pre > tc.NEG)).sum())
    assert removed, "typical_p never removed a token"
    return len(steps)


def sampled(**kw):
    return dict(dict(temperature=1.0, seed=11), **kw)


def minp1_subs():
    p = prompts(2)
    return [(p[0], sampled(fmt=VERDICT_SCHEMA, num_predict=40, min_p=1.0)),
            (p[1], sampled(fmt=None, num_predict=12, min_p=1.0, top_k=40, top_p=0.9, seed=5))]


def check_minp1(dev, monkeypatch, **cfg):
    """A temperature-1 request with min_p = 1 picks a maximal legal logit at every step (beside it, greedy would pick
    the smallest id among the maxima: the sampled request may pick any of them)."""
    eng = engine(dev, **cfg)
    rec = Recorder(eng, monkeypatch)
    reqs = run(eng, minp1_subs())
    n = sum(check_minp_request(rec, r, 1.0) for r in reqs)
    assert eng.stats["truncate_launches"] >= max(len(rec.steps(r)) for r in reqs) > 0
    print(f"min_p = 1: {n} recorded steps, every token at its row's legal maximum")
    return eng, reqs


def mixed_subs():
    """Slot 0: sampled with top-k / top-p only; then greedy ones; then the truncating ones (free grammar, fixed
    lengths, so that they live as long with their options as without)."""
    p = prompts(6, seed=9)
    return [(p[0], sampled(fmt=VERDICT_SCHEMA, num_predict=30, top_k=4, top_p=0.9, seed=3)),
            (p[1], dict(fmt=VERDICT_SCHEMA, num_predict=30)),
            (p[2], dict(fmt=None, num_predict=10)),
            (p[3], sampled(fmt=None, num_predict=14, min_p=0.3)),
            (p[4], sampled(fmt=None, num_predict=14, typical_p=0.5, seed=2)),
            (p[5], sampled(fmt=None, num_predict=14, typical_p=0.9, min_p=0.05, top_k=40, seed=7))]


def check_mixed(dev, monkeypatch, **cfg):
    subs = mixed_subs()
    eng = engine(dev, **cfg)
    rec = Recorder(eng, monkeypatch)
    on = run(eng, subs)
    assert eng.stats["truncate_launches"] > 0
    check_minp_request(rec, on[3], 0.3)
    check_typical_request(rec, on[4], 0.5)
    check_typical_request(rec, on[5], 0.9, minp=0.05)
    assert not rec.steps(on[0]) and not rec.steps(on[1]) and not rec.steps(on[2])
    monkeypatch.undo()
    off_eng = engine(dev, **cfg)
    off = run(off_eng, without_truncation(subs))
    assert off_eng.stats["truncate_launches"] == 0 and off_eng.s_minpln is None
    for a, b in zip(on[:3], off[:3]):
        assert a.out_ids == b.out_ids and a.text == b.text and a.done_reason == b.done_reason
    assert any(a.out_ids != b.out_ids for a, b in zip(on[3:], off[3:])), "truncation changed no sampled request"
    return eng, on


def check_never_asked(dev, **cfg):
    """Nobody asks (or asks at temperature 0, or with neutral values): no buffers, no launches, the old graph keys."""
    eng = engine(dev, **cfg)
    subs = without_truncation(mixed_subs())
    subs.append((subs[1][0], dict(fmt=None, num_predict=8, min_p=0.5, typical_p=0.5)))      # greedy: neutral
    subs.append((subs[1][0], sampled(fmt=None, num_predict=8, min_p=0.0, typical_p=1.0)))  # neutral values
    reqs = run(eng, subs)
    assert not any(r.truncates for r in reqs)
    assert eng.stats["truncate_launches"] == 0 and eng.s_minpln is None and eng.s_typ is None
    assert all("tr" not in k for k in eng._graphs)
    assert all(len(k) == 3 or (len(k) == 4 and k[3] == 1) or (len(k) == 5 and k[4] == "pen") for k in eng._graphs)
    return eng


def check_slot_reuse(dev):
    """A slot a truncating request leaves is reset for the plain sampled request that takes it."""
    p = prompts(2)
    eng = engine(dev, max_slots=1)
    first = eng.submit(p[0], **sampled(num_predict=10, min_p=1.0))
    eng.run_until_idle()
    launches = eng.stats["truncate_launches"]
    second = eng.submit(p[1], **sampled(num_predict=10))
    eng.run_until_idle()
    assert first.truncates and launches > 0 and eng.stats["truncate_launches"] == launches
    assert float(eng.s_minpln[0]) == tc.NEG and float(eng.s_typ[0]) == 1.0
    assert second.done_reason in ("stop", "length") and not second.truncates
