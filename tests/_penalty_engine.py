"""Shared engine-level penalty checks for tests/test_penalties_engine.py (CPU) and tests/test_penalties_engine_gpu.py.

Teacher-forced check.  For every output index i of every penalised (greedy) request, a fresh full-sequence forward
over prompt + out[:i] (a second engine without penalties, prefix cache and jump-forward, asked for one token, whose
sampler input is recorded), then the Python-loop penalty of tests/_penalty_cases.py over the true history (the last L
ids of prompt + out[:i], forced runs and pre-preemption output included), then the request's legal set (its grammar
walked over out[:i], and budget forcing), must have out[i] as its arg-max.

Positions whose top two penalised scores are closer than NOISE are skipped: the engine computed out[i] from a decode
step (or a jump's short prefill), the teacher from one prefill, and the two paths round differently.  Logits are bf16
on the GPU (relative precision 2^-8); 2^-6 of the larger of the two scores — four units in the last place — covers the
final rounding of both scores on both paths plus the few roundings a 2-layer model accumulates before it.  At most 10 %
of the positions of a scenario may be skipped."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _logprobs_cases import legal_mask  # noqa: E402
from _penalty_cases import oracle_row  # noqa: E402

from chronos import ops  # noqa: E402
from chronos.brain.engine.engine import DONE, Engine, EngineConfig  # noqa: E402
from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt  # noqa: E402
from chronos.sensor.replay import synthetic_chains  # noqa: E402

NOISE = 2.0 ** -6
MAX_SKIP = 0.10
W = 64
PEN_KEYS = ("repeat_penalty", "frequency_penalty", "presence_penalty", "repeat_last_n")


def engine(dev, **kw):
    base = dict(model="tiny", device=dev, max_slots=8, max_model_len=384, use_graphs=False, decode_burst=4,
                jump_forward=False, penalty_window=W)
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


def penalised(kw):
    return any(k in kw for k in PEN_KEYS[:3]) and kw.get("repeat_last_n", 64) != 0


def without_penalties(subs):
    return [(p, {k: v for k, v in kw.items() if k not in PEN_KEYS}) for p, kw in subs]


class Teacher:
    """Fresh forwards: ``logits(seqs)`` returns the last-position logits row (as the model produced it, on the host) of
    every token sequence, each prefilled from nothing by an engine that has no penalties."""

    def __init__(self, dev):
        self.eng = engine(dev, penalty_window=0, prefix_cache=False, max_slots=16, mixed_batching=False)
        self.rows = {}

    def logits(self, seqs):
        eng, real = self.eng, ops.constrained_sample

        def wrapped(logits, row_of_slot, next_tab, dist, done_state, state, *a, **k):
            if row_of_slot is not None:  # a prompt's first token (the decode bursts after it find every row DONE)
                owner = {r.slot: r for r in eng.prefilling}
                rows = row_of_slot.cpu().tolist()
                for slot, s in enumerate(state.cpu().tolist()):
                    if s > 0 and rows[slot] >= 0 and slot in owner:
                        self.rows[owner[slot].rid] = logits[rows[slot]].detach().cpu().clone()
            return real(logits, row_of_slot, next_tab, dist, done_state, state, *a, **k)

        ops.constrained_sample = wrapped
        try:
            reqs = [eng.submit(list(s), num_predict=1) for s in seqs]
            eng.run_until_idle()
        finally:
            ops.constrained_sample = real
        assert eng.stats["penalty_launches"] == 0
        return [self.rows.pop(r.rid) for r in reqs]


_TEACHERS = {}


def teacher(dev):
    """One teacher engine per device for the whole session (building an engine compiles its grammars)."""
    if dev not in _TEACHERS:
        _TEACHERS[dev] = Teacher(dev)
    return _TEACHERS[dev]


def teacher_check(eng, teacher, reqs, subs):
    """The teacher-forced check of every penalised request of ``reqs``; returns (positions checked, skipped)."""
    nxt, dist = eng.bank.next.cpu(), eng.bank.dist.cpu()
    V = nxt.shape[1]
    todo = [(r, kw) for r, (_, kw) in zip(reqs, subs) if penalised(kw)]
    assert todo
    seqs = [r.prompt_ids + r.out_ids[:i] for r, _ in todo for i in range(len(r.out_ids))]
    rows = iter(teacher.logits(seqs))
    checked = skipped = 0
    for r, kw in todo:
        assert kw.get("temperature", 0.0) == 0.0, "the teacher-forced check is for greedy requests"
        rp, fq, pr = (float(kw.get(k, d)) for k, d in zip(PEN_KEYS, (1.0, 0.0, 0.0)))
        last = kw.get("repeat_last_n", 64)
        L = eng.cfg.penalty_window if last < 0 else min(last, eng.cfg.penalty_window)
        assert r.penalty == (rp, fq, pr, L), r.penalty
        s = eng.bank.get(r.fmt).start
        # output indices the host appended as a grammar-forced run (jump-forward): part of the history of every later
        # step, legal, but not a sampler decision
        forced = {j for n0, k in r.meta.get("jump_spans", ()) for j in range(n0, n0 + k)}
        for i, tok in enumerate(r.out_ids):
            raw = next(rows)
            if i in forced:
                assert int(nxt[s, tok]) >= 0
                s = int(nxt[s, tok])
                continue
            score = raw.float()
            hist = (r.prompt_ids + r.out_ids[:i])[-L:]
            for t, v in oracle_row(score, hist, score.numel(), rp, fq, pr).items():
                score[t] = float(torch.tensor(float(v)).to(raw.dtype))  # written back in the row's dtype
            legal = legal_mask(nxt, dist, s, r.num_predict - i)
            score = torch.where(legal, score[:V], torch.tensor(float("-inf")))
            top = torch.topk(score, 2)
            a, b = float(top.values[0]), float(top.values[1])
            checked += 1
            if a - b < NOISE * max(abs(a), abs(b) if b > float("-inf") else 0.0):
                skipped += 1
                print(f"  near-tie: request {r.rid} index {i}: {a} vs {b}")
            else:
                assert int(top.indices[0]) == tok, (r.rid, i, tok, int(top.indices[0]), a, b)
            assert bool(legal[tok]), "the engine emitted an illegal token"
            s = int(nxt[s, tok])
    print(f"teacher-forced: {checked} positions, {skipped} skipped as near-ties")
    assert skipped <= MAX_SKIP * checked, (skipped, checked)
    return checked, skipped


PEN_A = dict(repeat_penalty=1.3, frequency_penalty=0.25, presence_penalty=0.5)
PEN_B = dict(repeat_penalty=1.5, repeat_last_n=16)
PEN_C = dict(presence_penalty=1.5, frequency_penalty=-0.125, repeat_last_n=-1)


def plain_subs():
    # (penalised requests are mostly grammar-constrained and short: in free text the tiny random model's top two
    # scores are within the noise at about one position in four, penalties or not)
    p = prompts(5)
    return [(p[0], dict(fmt=VERDICT_SCHEMA, num_predict=26, **PEN_A)),
            (p[1], dict(fmt=None, num_predict=12)),
            (p[2], dict(fmt=VERDICT_SCHEMA, num_predict=24, **PEN_B)),
            (p[3], dict(fmt=VERDICT_SCHEMA, num_predict=24, temperature=0.8, seed=3, top_k=4, top_p=0.9)),
            (p[4], dict(fmt="json", num_predict=14, **PEN_C)),
            (p[1], dict(fmt=None, num_predict=4, **PEN_A))]


def compaction_subs():
    p = prompts(12, seed=7)
    pens = (PEN_A, {}, PEN_B, {}, PEN_C, {})
    return [(q, dict(fmt=VERDICT_SCHEMA, num_predict=16 + 3 * (i % 4), **pens[i % 6]))
            for i, q in enumerate(p)]


def preemption_subs():
    chains = synthetic_chains(10, seed=21, native=False)
    return [(build_prompt(c.history), dict(fmt=VERDICT_SCHEMA, num_predict=20 + 2 * (i % 5),
                                           **(PEN_A if i % 2 else PEN_C)))
            for i, c in enumerate(chains)]


def preemption_blocks(dev, subs):
    """A quarter of the in-flight KV demand (tests/test_preemption.py)."""
    eng = engine(dev, kv_alloc="full", penalty_window=0)
    reqs = run(eng, without_penalties(subs))
    return 1 + sum(eng.blocks.blocks_for(len(r.prompt_ids) + r.num_predict) for r in reqs) // 4


def check_run(dev, subs, expect_stat=None, **cfg):
    eng = engine(dev, **cfg)
    reqs = run(eng, subs)
    if expect_stat:
        assert eng.stats[expect_stat] > 0, dict(eng.stats)
    assert eng.stats["penalty_launches"] > 0
    for r, (_, kw) in zip(reqs, subs):
        assert (r.penalty is not None) == penalised(kw)
    teacher_check(eng, teacher(dev), reqs, subs)
    return eng, reqs


def check_mixed(dev):
    """Prompts keep arriving while others decode (tests/test_mixed_batching.py); every other one is penalised."""
    p = prompts(8, seed=9)
    subs = [(q, dict(fmt=VERDICT_SCHEMA, num_predict=20, **(PEN_A if i % 2 else {}))) for i, q in enumerate(p)]
    eng = engine(dev, max_prefill_tokens=200, mixed_prefill_tokens=48, mixed_ratio=1)
    reqs = [eng.submit(q, **kw) for q, kw in subs[:3]]
    nxt = 3
    while eng.has_work() or nxt < len(subs):
        if nxt < len(subs) and eng.running:
            reqs.append(eng.submit(subs[nxt][0], **subs[nxt][1]))
            nxt += 1
        eng.step()
    assert eng.stats["mixed_steps"] > 0 and eng.stats["penalty_launches"] > 0
    teacher_check(eng, teacher(dev), reqs, subs)


def check_jump_forward(dev):
    """Jump-forward stays on beside penalties: the forced runs the host appends are in the history of later steps."""
    p = prompts(3)
    subs = [(p[0], dict(fmt=VERDICT_SCHEMA, num_predict=22, **PEN_A)),
            (p[1], dict(fmt=VERDICT_SCHEMA, num_predict=22, **PEN_C)),
            (p[2], dict(fmt=VERDICT_SCHEMA, num_predict=22))]
    eng = engine(dev, jump_forward=True, max_slots=4)
    reqs = run(eng, subs)
    assert eng.stats["jumps"] > 0 and eng.stats["penalty_launches"] > 0, dict(eng.stats)
    for r in reqs:
        assert set(json.loads(r.text)) == {"risk_score", "verdict", "reason"}
    spans = [sp for r in reqs[:2] for sp in r.meta.get("jump_spans", ())]
    assert spans and any(n0 + k < len(r.out_ids) for r in reqs[:2] for n0, k in r.meta.get("jump_spans", ())), \
        "a penalised request jumped, and sampled again after the run"
    teacher_check(eng, teacher(dev), reqs, subs)


PROPERTY_TOKENS = 24


def check_presence_property(dev):
    """No format, greedy, presence_penalty 100 over the engine's whole window (here wide enough for the whole
    sequence): the generated tokens are pairwise distinct and none is among the prompt's last W tokens — while the
    same request without the penalty, on the tiny random model, repeats."""
    wide = ops.MAX_PENALTY_WINDOW
    eng = engine(dev, penalty_window=wide)
    p = prompts(2)[1]
    base = eng.submit(p, num_predict=PROPERTY_TOKENS + 8)
    eng.run_until_idle()
    assert eng.stats["penalty_launches"] == 0 and eng.s_penpar is None
    out = base.out_ids[:PROPERTY_TOKENS]
    assert len(out) == PROPERTY_TOKENS and len(set(out)) < len(out), "the unpenalised run was chosen to repeat"
    r = eng.submit(p, num_predict=PROPERTY_TOKENS + 8, presence_penalty=100.0, repeat_last_n=-1)
    eng.run_until_idle()
    out = r.out_ids[:PROPERTY_TOKENS]
    assert r.penalty == (1.0, 0.0, 100.0, wide) and len(out) == PROPERTY_TOKENS
    assert len(r.prompt_ids) + PROPERTY_TOKENS <= wide
    assert len(set(out)) == len(out), out
    assert not set(out) & set(r.prompt_ids[-wide:])
    assert eng.stats["penalty_launches"] >= PROPERTY_TOKENS


def check_neutral_untouched(dev):
    """An unpenalised request beside penalised ones returns exactly what an engine without the feature returns; an
    engine that was never asked allocates and launches nothing, and its graph keys have the old form."""
    subs = plain_subs()
    on = run(engine(dev), subs)
    off_eng = engine(dev, penalty_window=0)
    off = run(off_eng, subs)  # penalties accepted, not applied
    assert not off_eng.can_penalise and all(r.penalty is None for r in off)
    assert off_eng.stats["penalty_launches"] == 0 and off_eng.s_penpar is None
    changed = 0
    for a, b, (_, kw) in zip(on, off, subs):
        if penalised(kw):
            changed += a.out_ids != b.out_ids
        else:
            assert a.out_ids == b.out_ids and a.text == b.text and a.done_reason == b.done_reason
    assert changed, "the penalised requests were chosen so that the penalties change their output"
    never = engine(dev)
    reqs = run(never, without_penalties(subs) + [(subs[0][0], dict(fmt=None, num_predict=8, repeat_penalty=1.5,
                                                                    repeat_last_n=0)),
                                                  (subs[0][0], dict(fmt=None, num_predict=8, repeat_penalty=1.0))])
    assert never.can_penalise and all(r.penalty is None for r in reqs)
    assert never.stats["penalty_launches"] == 0
    assert never.s_penpar is None and never.s_penlast is None and never.s_pentail is None and never.s_pentlen is None
    assert all(len(k) == 3 for k in never._graphs)
    for a, b in zip(reqs, off):
        assert a.out_ids == b.out_ids


def check_slot_reuse(dev):
    """A slot a penalised request leaves is reset for the unpenalised request that takes it."""
    p = prompts(2)
    eng = engine(dev, max_slots=1)
    first = eng.submit(p[0], num_predict=12, presence_penalty=100.0, repeat_last_n=-1)
    eng.run_until_idle()
    launches = eng.stats["penalty_launches"]
    second = eng.submit(p[1], num_predict=12)
    eng.run_until_idle()
    assert first.penalty and launches > 0 and eng.stats["penalty_launches"] == launches
    assert eng.s_penpar[0].tolist() == [1.0, 0.0, 0.0] and int(eng.s_penlast[0]) == 0
    off = engine(dev, max_slots=1, penalty_window=0)
    want = off.submit(p[1], num_predict=12)
    off.run_until_idle()
    assert second.out_ids == want.out_ids


def check_rejects_bad_window(dev):
    for bad in (-1, ops.MAX_PENALTY_WINDOW + 1):
        try:
            engine(dev, penalty_window=bad)
        except ValueError as e:
            assert "penalty_window" in str(e)
        else:
            raise AssertionError(f"penalty_window={bad} was accepted")
    assert DONE == 0
