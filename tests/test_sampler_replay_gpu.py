"""The sampled half of csrc/kernels/sampler.hip against the host replay of its noise stream
(tests/_sampler_cases.py): every sampled token is the fp64 argmax or within G of it, greedy rows are exact, idle slots
untouched, and the slot state advances as the cases' ``advance`` says for the device's token.

With CHRONOS_REPLAY_GAP_OUT set to a path, the largest gap among the rows where the device's token is not the fp64
argmax is written there per case (the record behind G, profiles/sampler/replay_gap.json)."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_GAPS = {}


def _record(name, gaps, rows):
    _GAPS[name] = {"max_gap": max((g for _, g in gaps), default=0.0), "disagreeing": len(gaps), "sampled_rows": rows}
    print(f"{name}: {len(gaps)} of {rows} sampled rows off the fp64 argmax, largest gap {_GAPS[name]['max_gap']:.3e}")
    out = os.environ.get("CHRONOS_REPLAY_GAP_OUT")
    if out:
        with open(out, "w") as fh:
            json.dump({"g_at_measurement": sc.G, "device": torch.cuda.get_device_name(0), "cases": _GAPS}, fh,
                      indent=1, sort_keys=True)
            fh.write("\n")


@pytest.mark.parametrize("kw", sc.GPU_CASES, ids=sc.case_id)
def test_one_step_follows_the_replay(kw):
    c = sc.Case(**kw)
    before, after = c.run(DEV)
    gaps = []
    try:
        c.check_step(before, after, sc.G, gaps=gaps)
    finally:
        _record(sc.case_id(kw), gaps, len(c.sampled()))
    assert len(c.sampled()) >= 90 and any(c.kinds[s] == "greedy" for s in range(c.n))


@pytest.mark.parametrize("vocab,dt", [(1003, "bf16"), (1024, "f32")])
def test_forty_steps_with_the_state_carried(vocab, dt):
    """Fresh logits every launch; the device's own state before the launch is what the replay starts from, so a
    near-tie decided the other way does not derail the comparison of the later steps."""
    c = sc.multi_step_case(vocab, dt)
    st = {k: v.to(DEV) for k, v in c.start().items()}
    gaps, judged = [], 0
    for step in range(40):
        buf = sc.step_logits(c, step)
        before = {k: v.cpu() for k, v in st.items()}
        judged += len(c.sampled(before))
        c.launch(DEV, st, buf.to(DEV))
        c.check_step(before, {k: v.cpu() for k, v in st.items()}, sc.G, buf=buf, gaps=gaps)
    _record(f"forty-steps-v{vocab}-{dt}", gaps, judged)
    state, nout = st["state"].cpu(), st["nout"].cpu()
    first = c.sampled()
    assert any(int(state[s]) == sc.DONE for s in first), "some sampled rows closed on the way"
    assert sum(int(nout[s]) == 40 for s in first) >= len(first) // 4, "and many were sampled at every step"


@pytest.mark.parametrize("vocab,hit", [(v, h) for v in (1003, 128256) for h in sc.OLD_HITS[v][:3 if v == 1003 else 1]],
                         ids=lambda p: str(p).replace(" ", ""))
def test_a_token_whose_hash_is_all_ones_does_not_win(vocab, hit):
    """(seed, nout, slot, token) with hash >> 8 == 2^24 - 1: the parent's u was 1.0f there, the score +inf, and the
    token won 30 below every other logit.  Fails on the parent of the u fix, passes with it."""
    c, tok = sc.forced_case(vocab, hit)
    s64 = c.scores(0)
    assert sc.top_two_gap(s64) > sc.G_CAP and int(s64.argmax()) != tok
    before, after = c.run(DEV)
    t = int(after["ring"][0, 0])
    assert t != tok, "the forced token won"
    assert t == int(s64.argmax())
    c.check_step(before, after, 0.0)


def test_engine_sampling_is_reproducible():
    """temperature 0.8 with a fixed seed on the ``small`` model: the same request twice on an idle engine gives the
    same tokens, and graph-replayed decode gives the tokens of eager decode.  ``slot`` is part of the noise key, so
    this reproducibility is per slot placement: an idle engine places the request in the same slot each time (the
    prefix cache is off, so the second run also computes the same prefill)."""
    from chronos.brain.engine.engine import Engine, EngineConfig
    from chronos.sensor.prompt import VERDICT_SCHEMA, build_prompt

    prompt = build_prompt(["[OPEN] attack_chain.sh -> /tmp/malware.bin", "[EXEC] attack_chain.sh -> curl"])
    outs = []
    for graphs in (True, False):
        eng = Engine(EngineConfig(model="small", device=DEV, max_slots=4, max_model_len=256, use_graphs=graphs,
                                  decode_burst=4, prefix_cache=False))
        runs = []
        for _ in range(2):
            reqs = [eng.submit(prompt, fmt=VERDICT_SCHEMA, num_predict=40, temperature=0.8, seed=1234),
                    eng.submit("free text", fmt=None, num_predict=24, temperature=0.8, seed=99, top_k=40, top_p=0.9)]
            eng.run_until_idle()
            assert all(r.error is None and r.out_ids for r in reqs)
            runs.append([list(r.out_ids) for r in reqs])
        assert runs[0] == runs[1], "same request, idle engine, same slots: same tokens"
        outs.append(runs[0])
    assert outs[0] == outs[1], "graph and eager decode"
    greedy = eng.submit(prompt, fmt=VERDICT_SCHEMA, num_predict=40)
    eng.run_until_idle()
    assert list(greedy.out_ids) != outs[1][0], "the sampled verdict is not the greedy one"
