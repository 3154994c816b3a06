"""The mid-M W4A16 MFMA GEMM (csrc/kernels/gemm_w4m.hip, OCP MXFP4 weights) against what chronos.ops runs today on the
same weights at M = 65 .. 512, per Llama-3-8B projection: the routed bf16 kernel on the dequantised copy (copy mode),
and one ``w4_expand`` launch plus that kernel (packed-only mode).

One process, modelled on scripts/bench_skinny_w4.py.  Per projection the epilogue the model uses: QKV plain with the
folded norm (NORMP), O and down the residual producer (kResid), gate_up SwiGLU + NORMP.  Candidates:

* every valid config x split-K (``ops/gemm.py`` ``_W4M`` / ``_w4m_valid``), screened with one timed pass each
  (``screen``); the ``--top`` fastest go on to the repeats;
* ``bf16_routed``: ``ops.linear`` / ``ops.gate_up_silu`` / ``ops.gemv_resid`` on ``.w`` with the same inputs;
* ``expand``: the same calls on a packed-only Q4Tensor with ``W4_MID = "off"`` — the expansion into the scratch and the
  bf16 kernel behind it, two launches.

Weights are cold: every launch takes the next of enough copies to exceed 600 MB (the MALL is 256 MB).  A pass is one
launch per copy (at least 40 launches) between two device events, replayed from a captured graph, so the figures are
kernel times.  The finalists and the two baselines are interleaved for ``--repeats`` passes; reported are the medians and
the [min, max] of the passes.  ``beats`` is the routing rule (``tests/test_mxfp4_skinny.py``'s: more than 3 % below the
baseline's median and the gap larger than both spreads together): 2 against the bf16 kernel on the copy, else 1 against
expansion + kernel, else 0.

    python scripts/bench_mid_w4.py --out profiles/mxfp4/mid_table.jsonl
    python scripts/bench_mid_w4.py --apply profiles/mxfp4/mid_table.jsonl   # table -> gemm_plan.json "w4mplans"
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("qkv_normp", 6144, 4096, 0), ("o_resid", 4096, 4096, 2), ("gate_up_swiglu_normp", 28672, 4096, 1),
          ("down_resid", 4096, 14336, 2)]
MS = [65, 80, 96, 128, 192, 256, 384, 512]
SPLITS = (1, 2, 4, 7, 8)
COLD_BYTES, MIN_LAUNCHES, MARGIN = 600e6, 40, 0.03
META = ("fused W4A16 MFMA GEMM for M = 65-512 (gemm_w4m.hip) for mxfp4 weights (Q4Tensor), rows [measured M, config id "
        "(-1 = lost to both baselines), split-K, beats] per N,K,epilogue: written by scripts/bench_mid_w4.py --apply "
        "from profiles/mxfp4/mid_table.jsonl; beats 2 = more than 3 % faster than the routed bf16 kernel on the "
        "resident copy by more than both spreads (routed in both weight modes), 1 = only faster than w4_expand + that "
        "kernel (routed for packed-only tensors); shapes and M without a row run the copy / the expansion")


def beats(rec) -> int:
    """The routing rule on one table record."""
    def win(base, spread):
        gap = rec[base] - rec["w4m_us"]
        s = (rec["w4m_spread_us"][1] - rec["w4m_spread_us"][0]) + (rec[spread][1] - rec[spread][0])
        return rec["w4m_us"] < (1 - MARGIN) * rec[base] and gap > s

    return 2 if win("bf16_routed_us", "bf16_spread_us") else 1 if win("expand_us", "expand_spread_us") else 0


def apply(table: str) -> None:
    """gemm_plan.json "w4mplans" from the table: per (N, K, mode) one row per measured M, [M, cfg, split-K, beats] where
    the kernel won against a baseline and [M, -1, 1, 0] where it lost to both (a row decides (previous M, M])."""
    from chronos.ops import gemm

    plan_path = os.path.join(os.path.dirname(os.path.abspath(gemm.__file__)), "gemm_plan.json")
    recs = [json.loads(line) for line in open(table) if line.strip()]
    out = {}
    for r in recs:
        b = beats(r)
        out.setdefault(f"{r['N']},{r['K']},{r['mode']}", []).append(
            [r["M"], r["w4m_cfg"], r["w4m_splitk"], b] if b else [r["M"], -1, 1, 0])
    for rows in out.values():
        rows.sort()
    with open(plan_path) as fh:
        plan = json.load(fh)
    plan["w4mplans"] = out
    plan.setdefault("meta", {})["w4mplans"] = META
    with open(plan_path, "w") as fh:
        json.dump(plan, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--apply", default=None, metavar="TABLE")
    ap.add_argument("--ms", type=int, nargs="*", default=MS)
    ap.add_argument("--kinds", nargs="*", default=[s[0] for s in SHAPES])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--top", type=int, default=2)
    a = ap.parse_args()
    if a.apply:
        return apply(a.apply)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_mid_w4.py measures GPU kernels: no GPU found")
    from chronos import ops
    from chronos.models.llama import Q4Tensor, quantize_mxfp4
    from chronos.ops import gemm
    from chronos.ops.gemm import LazyNorm

    ops.load()
    gemm.W4_MID = "off"  # the baselines are today's routes; the kernel under test is called directly
    k_ = torch.ops.chronos
    dev, bf = "cuda", torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(0)
    recs = []
    out = None
    if a.out:  # written point by point: an interrupted sweep keeps what it measured
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "w")

    def timed(fn, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    def captured(fn, n):
        """One pass as a graph (side-stream warm-up first: code objects, allocator, split-K tickets)."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for i in range(2):
                fn(i)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(n):
                fn(i)
        g.replay()
        return g

    def replayed(g, n):
        return timed(lambda i: g.replay() if i == 0 else None, 1) / n

    for kind, n, k, mode in SHAPES:
        if kind not in a.kinds:
            continue
        w0 = quantize_mxfp4((torch.randn(n, k, device=dev, generator=gen) * 0.02).to(bf))
        b16, b4 = 2 * n * k, n * k // 2 + n * k // 32
        c16 = max(2, int(-(-COLD_BYTES // b16)))
        c4 = max(2, int(-(-COLD_BYTES // b4)))
        w16 = [w0.w.clone() for _ in range(c16)]
        q4 = [(w0.q.clone(), w0.e.clone()) for _ in range(c4)]
        scratch = ops.W4Scratch(n * k, dev)
        packed = []
        for q, e in q4:
            t = Q4Tensor(q, e, None)
            t.scratch = scratch
            packed.append(t)
        n16, n4 = max(c16, MIN_LAUNCHES), max(c4, MIN_LAUNCHES)
        ones = torch.ones(k, device=dev, dtype=bf)
        for m in a.ms:
            s = (torch.randn(m, k, device=dev, generator=gen) + 0.1).to(bf)
            sf = s.float()
            part = torch.stack([(sf[:, i::8] ** 2).sum(1) for i in range(8)], 1).contiguous()
            resid = torch.randn(m, n, device=dev, generator=gen).to(bf) if mode == 2 else None
            pin = None if mode == 2 else part

            def w4m(cfg, sk):
                return lambda i: k_.gemm_w4m(s, q4[i % c4][0], q4[i % c4][1], mode, cfg, sk, resid, pin, 1e-5)

            def route(ws, c):
                if mode == 2:
                    return lambda i: ops.gemv_resid(s, ws[i % c], resid)
                if mode == 1:
                    return lambda i: ops.gate_up_silu(LazyNorm(s, part, ones, 1e-5), ws[i % c])
                return lambda i: ops.linear(LazyNorm(s, part, ones, 1e-5), ws[i % c])

            routed, expand = route(w16, c16), route(packed, c4)
            bplan = gemm.pp_plan(m, n, k, mode)
            screen = {}
            for cfg in sorted(gemm._W4M):
                for sk in SPLITS:
                    if gemm._w4m_valid(cfg, m, n, k, mode, sk):
                        g = captured(w4m(cfg, sk), n4)
                        screen[(cfg, sk)] = replayed(g, n4)
                        del g
            finalists = sorted(screen, key=screen.get)[:a.top]
            gb, ge = captured(routed, n16), captured(expand, n4)
            gs = {c: captured(w4m(*c), n4) for c in finalists}
            t = {c: [] for c in finalists}
            tb, te = [], []
            for _ in range(a.repeats):  # interleaved: one pass of each in turn
                tb.append(replayed(gb, n16))
                te.append(replayed(ge, n4))
                for c in finalists:
                    t[c].append(replayed(gs[c], n4))
            del gb, ge, gs
            best = min(finalists, key=lambda c: statistics.median(t[c]))
            med4, med16, mede = statistics.median(t[best]), statistics.median(tb), statistics.median(te)
            rec = dict(kind=kind, N=n, K=k, mode=mode, normp=mode != 2, M=m, copies_bf16=c16, copies_w4=c4,
                       repeats=a.repeats, timing="graph replay", bf16_plan=list(bplan) if bplan else None,
                       bf16_routed_us=round(med16, 2), bf16_spread_us=[round(min(tb), 2), round(max(tb), 2)],
                       expand_us=round(mede, 2), expand_spread_us=[round(min(te), 2), round(max(te), 2)],
                       w4m_cfg=best[0], w4m_splitk=best[1], w4m_us=round(med4, 2),
                       w4m_spread_us=[round(min(t[best]), 2), round(max(t[best]), 2)],
                       w4m_tbps=round(b4 / med4 / 1e6, 3), bf16_tbps=round(b16 / med16 / 1e6, 3),
                       vs_copy=round(med16 / med4, 3), vs_expand=round(mede / med4, 3),
                       finalists={f"{c[0]}/{c[1]}": round(statistics.median(v), 2) for c, v in t.items()},
                       screen={f"{c[0]}/{c[1]}": round(v, 2) for c, v in screen.items()})
            rec["beats"] = beats(rec)
            recs.append(rec)
            print(json.dumps(rec), flush=True)
            if out:
                out.write(json.dumps(rec) + "\n")
                out.flush()
        del w16, q4, packed, scratch
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
