"""Shared cases for the embedding tests (tests/test_embed.py on the CPU reference, tests/test_embed_gpu.py and
tests/test_embed_engine_gpu.py on the HIP kernels).

``pool_accum`` probe — exact integers.  Every row of ``s`` has exactly H/4 non-zero elements, each +-2^k with one k in
-3..3 per row, so the row's mean square is exactly 4^(k-1), its rsqrt 2^(1-k), and every normalised element is 0 or +-2
(eps = 0).  Row r's non-zero columns are those with (c + r) % 4 == 0 and the signs are a hash of (r, c), so every token
is identifiable, and the expected sums are integers whatever the order of summation.  Bound: |acc - e| <= n_tokens *
2^-20 per accumulator row — 2 ulp of rsqrt and one rounding of the product, per term of magnitude 2 (2 * 3 * 2^-24 <
2^-20).  ``MUTATIONS`` are the mistakes the probe must see, applied to the expectation; tests/test_embed.py proves that
each moves at least H/8 columns by at least 2.

``pool_finish`` probe — random accumulators and norm weights against fp64: |out - ref| <= 2^-12 |ref| + 2^-30 (an
fp32 sum of H <= 4096 squares is within H * 2^-24 relative in any order, the square root halves it, two more roundings
for the product and the quotient); at H = 8192 the bound is 2^-11.

Engine cases — ``embed_reference`` is one unchunked reference forward of the prompt's ids whose LM head is replaced by
the identity, so the "logits" are the final-RMSNorm hidden states of every token; the vector is g (.) their sum (or the
last one), L2-normalised in fp64.  Comparisons use the whole-model rule of tests/test_model_numerics_gpu.py: max |delta|
<= 2 % of the largest reference component (``CEILING``).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

CEILING = 0.02
ACCUM_H = (256, 4096)           # CPU; the GPU file adds 1024 and 8192
ACCUM_S = 8                     # accumulator rows
LENS = (1, 63, 64, 65, 129)     # rows per range: below, at and above a 64-row boundary, and several segments
MUTATIONS = ("drop", "double", "neighbour", "shift", "swap_sel", "overwrite")


def _sign(r: np.ndarray, c: np.ndarray) -> np.ndarray:
    h = (r.astype(np.uint64) * np.uint64(0x9E3779B1)) ^ (c.astype(np.uint64) * np.uint64(0x85EBCA77))
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(12)
    return np.where((h & np.uint64(1)) == 1, 1.0, -1.0)


def probe_rows(T: int, H: int) -> tuple[torch.Tensor, np.ndarray]:
    """(s [T, H] bf16, the exact normalised rows [T, H] float64: 0 or +-2)."""
    r, c = np.arange(T)[:, None], np.arange(H)[None, :]
    on = ((c + r) % 4) == 0
    sg = _sign(np.broadcast_to(r, (T, H)), np.broadcast_to(c, (T, H)))
    k = (np.arange(T) * 5 + 2) % 7 - 3  # -3..3, every value
    s = np.where(on, sg * (2.0 ** k)[:, None], 0.0)
    return torch.tensor(s, dtype=torch.float32).to(torch.bfloat16), np.where(on, 2.0 * sg, 0.0)


def accum_case(H: int) -> dict:
    """Two pool_accum calls over one ``s``.  Call 0: seven sequences — ranges of 1, 63, 64 rows, an empty range, a
    skipped 10-row sequence in the middle (sel -1), then 65 and 129 rows — with a non-identity ``sel``; call 1: second
    chunks of 17 and 40 rows for two of them, into the same accumulator rows.  A NaN-filled row follows every
    sequence's rows, inside no range, so a kernel that reads one row too many poisons its sums."""
    lens0 = [1, 63, 64, 0, 10, 65, 129]
    sel0 = [5, 0, 3, 6, -1, 2, 7]
    lens1 = [17, 40]
    sel1 = [0, 7]
    q0, q1, at, nan_rows = [], [], 0, []
    for n in lens0:
        q0.append((at, at + n))
        nan_rows.append(at + n)
        at += n + 1
    for n in lens1:
        q1.append((at, at + n))
        nan_rows.append(at + n)
        at += n + 1
    s, xn = probe_rows(at, H)
    s[nan_rows] = float("nan")
    xn[nan_rows] = np.nan
    return dict(H=H, s=s, xn=xn, calls=[(q0, sel0), (q1, sel1)], nan_rows=nan_rows)


def accum_expected(case: dict, mutate: str | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(expected accumulators [ACCUM_S, H] float64 — exact integers —, pooled tokens per accumulator row).  ``mutate``
    applies one of MUTATIONS to the computation."""
    assert mutate is None or mutate in MUTATIONS
    xn = np.nan_to_num(case["xn"], nan=0.0) if mutate in ("neighbour", "shift") else case["xn"]
    e = np.zeros((ACCUM_S, case["H"]))
    ntok = np.zeros(ACCUM_S)
    for ci, (q, sel) in enumerate(case["calls"]):
        sel = list(sel)
        if mutate == "swap_sel" and ci == 0:
            sel[1], sel[2] = sel[2], sel[1]
        for b, ((lo, hi), row) in enumerate(zip(q, sel)):
            if row < 0 or hi <= lo:
                continue
            rows = list(range(lo, hi))
            if ci == 0 and b == 1:  # the 63-row sequence takes the token mutations
                if mutate == "drop":
                    del rows[7]
                elif mutate == "double":
                    rows.append(rows[7])
                elif mutate == "neighbour":
                    rows.append(q[2][0])  # the first token of the sequence after it
                elif mutate == "shift":
                    rows = list(range(lo + 1, hi + 1))
            add = xn[rows].sum(0)
            if mutate == "overwrite" and ci == 1:
                e[row] = add
            else:
                e[row] += add
            ntok[row] += len(rows)
    return e, ntok


def run_accum(case: dict, device, fn) -> torch.Tensor:
    """``fn`` = ops.pool_accum; returns the accumulators [ACCUM_S, H] fp32 (on ``device``) after both calls."""
    acc = torch.zeros(ACCUM_S, case["H"], dtype=torch.float32, device=device)
    s = case["s"].to(device)
    for q, sel in case["calls"]:
        fn(s, 0.0, torch.tensor(q, dtype=torch.int32, device=device).view(-1, 2),
           torch.tensor(sel, dtype=torch.int32, device=device), acc)
    return acc


def check_accum(acc: torch.Tensor, case: dict) -> float:
    e, ntok = accum_expected(case)
    d = np.abs(acc.double().cpu().numpy() - e)
    assert np.isfinite(d).all(), "non-finite accumulator: a row outside every range was read"
    bound = ntok[:, None] * 2.0 ** -20
    worst = float((d - bound).max())
    print(f"pool_accum H={case['H']}: max |acc - e| = {d.max():.3g} (bound {bound.max():.3g})")
    assert (d <= bound).all(), f"H={case['H']}: |acc - e| exceeds n_tokens * 2^-20 by {worst:.3g}"
    return float(d.max())


def moved_columns(case: dict, mutate: str) -> int:
    """Columns of the accumulator row a mutation hits hardest that it moves by at least 2."""
    e, _ = accum_expected(case)
    m, _ = accum_expected(case, mutate)
    return int((np.abs(m - e) >= 2.0).sum(1).max())


# ---- pool_finish ------------------------------------------------------------------------------------------------------
def finish_rel(H: int) -> float:
    return 2.0 ** -11 if H > 4096 else 2.0 ** -12


def finish_case(H: int, seed: int = 0) -> dict:
    g = torch.Generator().manual_seed(1000 + H + seed)
    acc = torch.randn(ACCUM_S, H, generator=g) * 37.0
    acc[4] = 0.0  # a zero row gives zeros
    w = (1.0 + 0.5 * torch.rand(H, generator=g) - 0.25).to(torch.bfloat16)
    rows = [6, 4, 0, 3]  # not all of them, not in order
    return dict(H=H, acc=acc, g=w, rows=rows)


def finish_expected(case: dict, mutate: str | None = None) -> np.ndarray:
    acc, w = case["acc"].double().numpy(), case["g"].double().numpy()
    out = []
    for r in case["rows"]:
        v = acc[r] * (1.0 if mutate == "no_g" else w)
        n = np.sqrt((v * v).sum())
        out.append(v if mutate == "no_norm" else (v / n if n > 0 else np.zeros_like(v)))
    return np.stack(out)


def finish_ok(out: np.ndarray, case: dict) -> bool:
    ref = finish_expected(case)
    return bool((np.abs(out - ref) <= finish_rel(case["H"]) * np.abs(ref) + 2.0 ** -30).all())


def run_finish(case: dict, device, fn) -> tuple[torch.Tensor, torch.Tensor]:
    """``fn`` = ops.pool_finish; returns (out [n, H], the accumulators afterwards)."""
    acc = case["acc"].clone().to(device)
    out = torch.full((len(case["rows"]), case["H"]), float("nan"), dtype=torch.float32, device=device)
    fn(acc, torch.tensor(case["rows"], dtype=torch.int32, device=device), case["g"].to(device), out)
    return out, acc


def check_finish(case: dict, device, fn) -> None:
    out, acc = run_finish(case, device, fn)
    o = out.double().cpu().numpy()
    ref = finish_expected(case)
    rel = np.abs(o - ref).max() / np.abs(ref).max()
    print(f"pool_finish H={case['H']}: max |out - ref| / max |ref| = {rel:.3g}")
    assert finish_ok(o, case), f"H={case['H']}: pool_finish outside {finish_rel(case['H']):.3g} |ref| + 2^-30"
    assert (o[1] == 0).all(), "a zero accumulator row must give zeros"
    acc = acc.cpu()
    assert (acc[case["rows"]] == 0).all(), "listed accumulator rows must be zero afterwards"
    rest = [r for r in range(ACCUM_S) if r not in case["rows"]]
    assert torch.equal(acc[rest], case["acc"][rest]), "unlisted accumulator rows must stay"


# ---- engine -----------------------------------------------------------------------------------------------------------
PROMPT_LENS = (1, 15, 16, 17, 70)  # around the 16-token block, and several 32-token chunks


def prompts(vocab: int = 1000, seed: int = 11, lens=PROMPT_LENS) -> list[list[int]]:
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(3, vocab, (n,), generator=g).tolist() for n in lens]


def randomise_final_norm(model, seed: int = 5) -> None:
    """Random-init models store ones as the final norm weight; give ``final_norm`` real values (the LM head, which a
    loader would have folded them into, plays no part in an embedding) so a vector that ignores it is wrong."""
    g = torch.Generator().manual_seed(seed)
    w = (1.0 + torch.rand(model.cfg.hidden_size, generator=g) - 0.5).to(torch.bfloat16)
    model.w.final_norm = w.to(model.w.norm.device)


def cpu_copy(model_gpu):
    """A CPU model with the GPU model's weights (as tests/test_model_numerics_gpu.py copies them)."""
    from chronos.models.llama import build_model

    mc = build_model(model_gpu.cfg, "cpu", seed=0, max_position=model_gpu.cos_sin.shape[0])
    for lg, lc in zip(model_gpu.w.layers, mc.w.layers):
        for n in ("attn_norm", "wqkv", "wo", "mlp_norm", "w_gu", "w_down"):
            getattr(lc, n).copy_(getattr(lg, n).cpu())
    mc.w.embed.copy_(model_gpu.w.embed.cpu())
    if mc.w.lm_head is not mc.w.embed:
        mc.w.lm_head.copy_(model_gpu.w.lm_head.cpu())
    mc.w.norm.copy_(model_gpu.w.norm.cpu())
    mc.w.final_norm = model_gpu.w.final_norm.cpu().clone()
    return mc


def make_engine(device: str, model=None, preset: str = "tiny", tokenizer=None, **kw):
    from chronos.brain.engine.engine import Engine, EngineConfig

    args = dict(model=preset, device=device, max_slots=4, block_size=16, max_model_len=128, max_prefill_tokens=32,
                prefill_ramp=0, warm_formats=(), seed=3)
    args.update(kw)
    return Engine(EngineConfig(**args), model=model, tokenizer=tokenizer)


def embed_reference(model, ids: list[int], pooling: str) -> torch.Tensor:
    """The embedding of ``ids`` from one unchunked reference forward on the CPU: the LM head is replaced by the
    identity (the final norm weight the forward applies is ones), so the forward returns the final-RMSNorm hidden state
    of every token; fp64 from there on."""
    from chronos.models.llama import KVCache, LlamaModel, make_prefill_batch

    w = model.w
    assert w.norm.device.type == "cpu" and bool((w.norm == 1).all())
    d = model.cfg.hidden_size
    eye = dataclasses.replace(w, lm_head=torch.eye(d, dtype=torch.bfloat16))
    m = LlamaModel(model.cfg, eye, model.tp, "cpu", max_position=model.cos_sin.shape[0])
    nb = (len(ids) + 15) // 16
    kv = KVCache(model.cfg, model.tp, nb + 1, 16, "cpu")
    sb = make_prefill_batch([ids], [0], [list(range(1, nb + 1))], model.cfg, model.tp, "cpu")
    sb.last_idx = torch.arange(len(ids), dtype=torch.int64)
    xh = m.forward(sb, kv, logits_dtype=torch.float32).double()  # [T, d]
    v = (xh.sum(0) if pooling == "mean" else xh[-1]) * w.final_norm.double()
    return (v / v.norm()).float()


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |delta| as a fraction of the largest reference component (the whole-model rule; CEILING = 0.02)."""
    return float((got.double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max())


def embed_all(eng, ps, pooling=None, one_at_a_time: bool = False, **kw) -> list:
    reqs = []
    for p in ps:
        reqs.append(eng.submit_embed(p, pooling=pooling, **kw))
        if one_at_a_time:
            eng.run_until_idle()
    eng.run_until_idle()
    for r in reqs:
        assert r.done_reason == "embed" and r.error is None, (r.done_reason, r.error)
        assert r.embedding.device.type == "cpu" and r.embedding.dtype == torch.float32
    return reqs


def assert_idle(eng, free_blocks: int) -> None:
    assert not eng.has_work()
    assert sorted(eng.free_slots) == list(range(eng.cfg.max_slots))
    assert eng.blocks.free == free_blocks
    assert not eng.waiting and not eng.prefilling and not eng.running and not eng._embed_pending
    if eng.s_pool is not None:
        assert float(eng.s_pool.abs().max()) == 0.0, "accumulator rows must be zero between requests"
