"""Embedding requests through the engine on the GPU (``tiny`` and ``small``, HIP kernels) against the CPU reference
engine on the same weights, copied as tests/test_model_numerics_gpu.py copies them.  Every comparison uses that file's
whole-model rule: max |delta| <= 2 % of the largest reference component.

Measured on an MI355X (fraction of the largest reference component, worst over the five prompts; ceiling 0.02):
tiny 0.0036 (mean) / 0.0096 (last), small 0.0066 (mean) / 0.0146 (last); in one 4096-token chunk 0.0096 (tiny) /
0.0127 (small); mixed steps against the embed-alone run 0.0000.

fp8 KV cache: measured ABOVE the ceiling before the engine refused the combination — tiny 0.0200 .. 0.0463 (mean) /
0.0230 .. 0.0435 (last), small 0.0384 .. 0.0533 (mean) / 0.0431 .. 0.0625 (last).  That is the cache format, not the
pooling: e4m3 keeps three mantissa bits, so every stored K / V element is off by up to 2^-4 of itself, and a one-token
prompt's attention output is exactly its own rounded V (0.0399 / 0.0431 at length 1).  The bound is not widened for
it: an engine with an fp8 KV cache does not serve embeddings (``test_fp8_kv``), and the README says so.
"""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _embed_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


PRESETS = ("tiny", "small")
_pairs: dict = {}


def _pair(preset):
    """(GPU engine, CPU engine on the same weights, prompts, CPU-engine vectors per pooling mode), built once."""
    if preset not in _pairs:
        eg = C.make_engine(DEV, preset=preset)
        C.randomise_final_norm(eg.model)
        ec = C.make_engine("cpu", model=C.cpu_copy(eg.model), tokenizer=eg.tok, preset=preset)
        ps = C.prompts()
        ref = {m: [r.embedding for r in C.embed_all(ec, ps, m)] for m in ("mean", "last")}
        _pairs[preset] = (eg, ec, ps, ref)
    return _pairs[preset]


@pytest.fixture(params=PRESETS)
def pair(request):
    return _pair(request.param)


@pytest.mark.parametrize("pooling", ["mean", "last"])
@pytest.mark.parametrize("one_at_a_time", [False, True])
def test_gpu_engine_equals_cpu_reference_engine(pair, pooling, one_at_a_time):
    eg, ec, ps, ref = pair
    eg.blocks.clear_cache()
    free = eg.blocks.free
    reqs = C.embed_all(eg, ps, pooling, one_at_a_time)
    torch.cuda.synchronize()
    for p, r, e in zip(ps, reqs, ref[pooling]):
        err = C.rel_err(r.embedding, e)
        print(f"{eg.cfg.model} {pooling} len {len(p)}: max |d| / max |ref| = {err:.4f}")
        assert abs(float(r.embedding.double().norm()) - 1.0) <= 1e-3
        assert err <= C.CEILING
    C.assert_idle(eg, free)
    assert not eg._graphs, "an embedding request captures no decode graph"


def test_chunk_invariance_on_the_gpu(pair):
    eg, ec, ps, ref = pair
    big = C.make_engine(DEV, model=eg.model, tokenizer=eg.tok, preset=eg.cfg.model, max_prefill_tokens=4096)
    for m in ("mean", "last"):
        for r, e in zip(C.embed_all(big, ps, m), ref[m]):
            err = C.rel_err(r.embedding, e)
            print(f"{eg.cfg.model} one chunk {m} len {len(r.prompt_ids)}: {err:.4f}")
            assert err <= C.CEILING


def test_accounting_on_the_gpu(pair):
    eg = pair[0]
    eg.blocks.clear_cache()
    free = eg.blocks.free
    ps = C.prompts(seed=31, lens=[5 + 7 * i for i in range(3 * eg.cfg.max_slots)])
    reqs = [eg.submit_embed(p, pooling="last" if i % 2 else "mean") for i, p in enumerate(ps)]
    eg.run_until_idle()
    assert [r.done_reason for r in reqs] == ["embed"] * len(ps)
    eg.blocks.clear_cache()
    C.assert_idle(eg, free)


def test_mixed_steps_on_the_gpu():
    """Embed requests arrive while JSON-constrained requests decode: those finish with valid JSON, and the vectors agree
    with the embed-alone run within the ceiling.  (One preset: the scheduling path does not depend on the model size,
    and the JSON automaton takes seconds to compile.)"""
    eg, ec, ps, ref = _pair("tiny")
    alone = [r.embedding for r in C.embed_all(eg, ps, "mean")]
    e = C.make_engine(DEV, model=eg.model, tokenizer=eg.tok, decode_burst=1, max_slots=8)
    gens = [e.submit(p, fmt="json", num_predict=48, raw=True) for p in ('{"a": 1}', "[1, 2, 3]")]
    for _ in range(4):
        e.step()
    assert e.running
    embs = [e.submit_embed(p) for p in ps]
    e.run_until_idle()
    torch.cuda.synchronize()
    assert e.stats["mixed_steps"] > 0
    for g in gens:
        assert g.done_reason in ("stop", "length"), (g.done_reason, g.error)
        json.loads(g.text)
    for r, a in zip(embs, alone):
        assert r.done_reason == "embed"
        err = C.rel_err(r.embedding, a)
        print(f"mixed len {len(r.prompt_ids)}: {err:.4f}")
        assert err <= C.CEILING


def test_fp8_kv(pair):
    """The same engine with an fp8 KV cache.  Its vectors were measured 0.0200 .. 0.0463 (tiny) and 0.0384 .. 0.0625
    (small) of the largest component off the bf16-KV CPU reference, above the ceiling (module docstring), so the engine
    serves no embeddings in that mode: both pooling modes finish with the error, nothing is allocated or launched for
    them, and the engine goes on generating."""
    eg, ec, ps, ref = pair
    e8 = C.make_engine(DEV, model=eg.model, tokenizer=eg.tok, preset=eg.cfg.model, kv_dtype="fp8")
    free = e8.blocks.free
    done = []
    for m in ("mean", "last"):
        for p in ps:
            r = e8.submit_embed(p, pooling=m, callback=done.append)
            assert r.done_reason == "error" and r.embedding is None
            assert r.error == "embeddings are served with a bf16 KV cache only, not kv_dtype='fp8'"
    assert len(done) == 2 * len(ps) and e8.s_pool is None
    C.assert_idle(e8, free)
    g = e8.submit(ps[3], num_predict=4)
    e8.run_until_idle()
    torch.cuda.synchronize()
    assert g.done_reason in ("stop", "length") and g.out_ids and e8.stats["embed_requests"] == 0
