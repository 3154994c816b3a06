"""Shared engine-level logprob checks for tests/test_logprobs_engine.py (CPU) and tests/test_logprobs_engine_gpu.py.

A recorder wraps ``ops.constrained_sample`` and clones, at every (eager) call, the logits row, grammar state and
remaining budget of every slot that wants logprobs.  Every entry the engine reports must equal the formula of
tests/_logprobs_cases.py ``expected`` on those recorded inputs: ids exact, logprobs to 1e-3 absolute (same reasoning as
there: exact fp32 inputs, only summation order and the exp / log intrinsics differ)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _logprobs_cases import TOL, expected, legal_mask  # noqa: E402

from chronos import ops  # noqa: E402
from chronos.brain.engine.engine import Engine, EngineConfig  # noqa: E402
from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt  # noqa: E402
from chronos.sensor.replay import synthetic_chains  # noqa: E402


def engine(dev, **kw):
    base = dict(model="tiny", device=dev, max_slots=8, max_model_len=384, use_graphs=False, decode_burst=4,
                jump_forward=False, max_logprobs=5)
    base.update(kw)
    return Engine(EngineConfig(**base))


def prompts(n, seed=4):
    return [build_prompt(c.history) for c in synthetic_chains(n, seed=seed, native=False)]


class Recorder:
    """{(request id, output index): (logits row fp32 on the host, grammar state, remaining)} of every sampler call."""

    def __init__(self, eng, monkeypatch):
        self.eng, self.rec = eng, {}
        real = ops.constrained_sample

        def wrapped(logits, row_of_slot, next_tab, dist, done_state, state, remaining, temperature, seed, ids, pos,
                    ctx, nout, *a, **k):
            self.note(logits, row_of_slot, state, remaining, nout)
            return real(logits, row_of_slot, next_tab, dist, done_state, state, remaining, temperature, seed, ids,
                        pos, ctx, nout, *a, **k)

        monkeypatch.setattr(ops, "constrained_sample", wrapped)

    def note(self, logits, row_of_slot, state, remaining, nout):
        eng = self.eng
        owner = {r.slot: r for r in (*eng.prefilling, *eng.running.values())}
        st, rem, no = state.cpu().tolist(), remaining.cpu().tolist(), nout.cpu().tolist()
        rows = row_of_slot.cpu().tolist() if row_of_slot is not None else list(range(len(st)))
        V = eng.bank.next.shape[1]
        for slot, s in enumerate(st):
            r = owner.get(slot)
            if s <= 0 or rows[slot] < 0 or r is None or r.logprobs < 0:
                continue
            key = (r.rid, len(r.resume_out) + no[slot])
            assert key not in self.rec, "an output index was sampled twice"
            self.rec[key] = (logits[rows[slot], :V].float().cpu().clone(), s, rem[slot])


def check_request(eng, rec, r):
    """Every reported entry of request r against the recorded sampler inputs; returns the largest logprob error."""
    assert r.done_reason in ("stop", "length"), (r.done_reason, r.error)
    assert len(r.out_logprobs) == len(r.out_ids) > 0
    nxt, dist = eng.bank.next.cpu(), eng.bank.dist.cpu()
    worst = 0.0
    for i, (lp, top) in enumerate(r.out_logprobs):
        row, s, rem = rec.rec[(r.rid, i)]
        legal = legal_mask(nxt, dist, s, rem)
        lse, e_ids, e_vals = expected(row, legal, max(r.logprobs, 1))
        e_ids, e_lp = e_ids[:r.logprobs], (e_vals - lse)[:r.logprobs]
        keep = e_ids >= 0
        assert [t for t, _ in top] == e_ids[keep].tolist(), (r.rid, i)
        got = torch.tensor([lp] + [v for _, v in top])
        want = torch.cat([(row[r.out_ids[i]] - lse).reshape(1), e_lp[keep]])
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got), fin)
        if bool(fin.any()):
            worst = max(worst, float((got[fin] - want[fin]).abs().max()))
        if int(legal.sum()) == 1:
            assert lp == 0.0, "a forced token must have logprob exactly 0.0"
        if r.temperature == 0.0 and r.logprobs > 0:  # greedy: the chosen token is the first alternative
            assert top[0][0] == r.out_ids[i] and top[0][1] == lp
    assert worst <= TOL, worst
    return worst


def run(eng, subs):
    """subs: (prompt, kwargs of Engine.submit)."""
    reqs = [eng.submit(p, **kw) for p, kw in subs]
    eng.run_until_idle()
    return reqs


def without_logprobs(subs):
    return [(p, {k: v for k, v in kw.items() if k != "logprobs"}) for p, kw in subs]


def check_run(dev, monkeypatch, subs, expect_stat=None, **cfg):
    """Run ``subs`` with a recorder, check every wanted request, and compare the tokens with a run that asks for no
    logprobs (jump_forward is off in both)."""
    eng = engine(dev, **cfg)
    rec = Recorder(eng, monkeypatch)
    reqs = run(eng, subs)
    if expect_stat:
        assert eng.stats[expect_stat] > 0, dict(eng.stats)
    assert eng.stats["logprob_launches"] > 0
    worst = 0.0
    for r, (_, kw) in zip(reqs, subs):
        if kw.get("logprobs", -1) >= 0:
            assert r.logprobs == min(kw["logprobs"], eng.cfg.max_logprobs)
            worst = max(worst, check_request(eng, rec, r))
        else:
            assert r.out_logprobs == []
    print(f"largest |logprob - expected| over {len(rec.rec)} recorded steps: {worst:.2e}")
    monkeypatch.undo()
    off = engine(dev, **cfg)
    base = run(off, without_logprobs(subs))
    assert off.stats["logprob_launches"] == 0 and off.s_lp is None
    for a, b in zip(reqs, base):
        assert a.out_ids == b.out_ids and a.text == b.text and a.done_reason == b.done_reason
    return eng, reqs


def plain_subs():
    p = prompts(4)
    return [(p[0], dict(fmt=VERDICT_SCHEMA, num_predict=24, logprobs=3)),
            (p[1], dict(fmt=None, num_predict=8, logprobs=0)),
            (p[2], dict(fmt="json", num_predict=12, logprobs=9)),  # clamped to max_logprobs
            (p[3], dict(fmt=VERDICT_SCHEMA, num_predict=20, temperature=0.8, seed=3, top_k=4, top_p=0.9, logprobs=2))]


def compaction_subs():
    p = prompts(12, seed=7)
    return [(q, dict(fmt=VERDICT_SCHEMA, num_predict=18 + 6 * (i % 5), logprobs=i % 4)) for i, q in enumerate(p)]


def preemption_subs():
    chains = synthetic_chains(10, seed=21, native=False)
    return [(build_prompt(c.history), dict(fmt=VERDICT_SCHEMA, num_predict=24 + 4 * (i % 5), logprobs=2))
            for i, c in enumerate(chains)]


def preemption_blocks(dev, subs):
    """A quarter of the in-flight KV demand (tests/test_preemption.py)."""
    eng = engine(dev, kv_alloc="full")
    reqs = run(eng, without_logprobs(subs))
    return 1 + sum(eng.blocks.blocks_for(len(r.prompt_ids) + r.num_predict) for r in reqs) // 4


def mixed_subs():
    p = prompts(10, seed=9)
    return [(q, dict(fmt=VERDICT_SCHEMA, num_predict=30, **({"logprobs": 3} if i % 2 else {})))
            for i, q in enumerate(p)]


def check_mixed(dev, monkeypatch):
    """Prompts keep arriving while others decode (tests/test_mixed_batching.py); every other one wants logprobs."""
    subs = mixed_subs()

    def drive(eng, subs):
        reqs = [eng.submit(p, **kw) for p, kw in subs[:3]]
        nxt = 3
        while eng.has_work() or nxt < len(subs):
            if nxt < len(subs) and eng.running:
                reqs.append(eng.submit(subs[nxt][0], **subs[nxt][1]))
                nxt += 1
            eng.step()
        return reqs

    cfg = dict(max_prefill_tokens=200, mixed_prefill_tokens=48, mixed_ratio=1)
    eng = engine(dev, **cfg)
    rec = Recorder(eng, monkeypatch)
    reqs = drive(eng, subs)
    assert eng.stats["mixed_steps"] > 0 and eng.stats["logprob_launches"] > 0
    for r, (_, kw) in zip(reqs, subs):
        if "logprobs" in kw:
            check_request(eng, rec, r)
        else:
            assert r.out_logprobs == []
    monkeypatch.undo()
    base = drive(engine(dev, **cfg), without_logprobs(subs))
    for a, b in zip(reqs, base):
        assert a.out_ids == b.out_ids


def check_jump_suppressed(dev):
    eng = engine(dev, jump_forward=True, max_slots=4)
    p = prompts(2)
    base = eng.submit(p[0], fmt=VERDICT_SCHEMA, num_predict=60)
    eng.run_until_idle()
    assert eng.stats["jumps"] > 0, "the schema has forced runs: without logprobs the engine jumps over them"
    j0 = eng.stats["jumps"]
    r = eng.submit(p[0], fmt=VERDICT_SCHEMA, num_predict=60, logprobs=2)
    eng.run_until_idle()
    assert eng.stats["jumps"] == j0, "jump-forward must be suppressed while a request wants logprobs"
    assert set(json.loads(r.text)) == {"risk_score", "verdict", "reason"}
    assert len(r.out_logprobs) == len(r.out_ids)
    assert json.loads(base.text) is not None


def check_never_asked(dev):
    eng = engine(dev)
    reqs = run(eng, without_logprobs(plain_subs()))
    assert all(r.done_reason in ("stop", "length") and r.out_logprobs == [] for r in reqs)
    assert eng.stats["logprob_launches"] == 0
    assert eng.s_lp is None and eng.s_lpids is None and eng.s_lpwant is None and eng._snap_lp is None
    assert all(len(k) == 3 for k in eng._graphs)
    off = engine(dev, max_logprobs=0)  # the feature does not exist: a request that asks is served without
    r = off.submit(prompts(1)[0], fmt=VERDICT_SCHEMA, num_predict=30, logprobs=3)
    off.run_until_idle()
    assert r.done_reason in ("stop", "length") and r.logprobs == -1 and r.out_logprobs == []
    assert off.stats["logprob_launches"] == 0 and off.s_lp is None
