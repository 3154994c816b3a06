"""The W4A16 mode of the skinny MFMA GEMM (csrc/kernels/gemm_skinny.hip, OCP MXFP4 weights) against what chronos.ops
runs on the dequantised bf16 copy of the same weights, per Llama-3-8B projection at M = 2 .. 64.

One process.  Per projection the epilogue the model uses above the GEMV's M: QKV plain with the folded norm (NORMP),
O and down the residual producer (kResid), gate_up SwiGLU + NORMP.  Candidates:

* every valid W4 config x split-K (``ops/gemm.py`` ``_SK4`` / ``_sk4_valid``), screened with one timed pass each; the
  ``--top`` fastest go on to the repeats;
* ``bf16_routed``: ``ops.linear`` / ``ops.gate_up_silu`` / ``ops.gemv_resid`` on ``.w`` with the same inputs — the
  plan's kernel for that M, which is what the model runs today.

Weights are cold: every launch takes the next of enough copies to exceed 600 MB (the MALL is 256 MB).  A pass is one
launch per copy (at least 40 launches) between two device events.  Every pass that counts is the replay of a captured
graph of those launches, so the figures are kernel times: at 6-15 us per launch an eager host loop (the W4 side a raw
op call, the bf16 side the Python wrappers with their plan look-up and LazyNorm) can be slower than the device and
would time the host instead.  The finalists and the routed bf16 kernel are interleaved for ``--repeats`` passes;
reported are the medians and the [min, max] of the passes, and next to them the same passes issued eagerly
(``*_eager_us``) to show where the host loop would have set the time.  ``w4_wins`` is the routing rule on the graph
figures: the best W4 median is more than 3 % below the bf16 median and the gap is larger than both spreads together.

    python scripts/bench_skinny_w4.py --out profiles/mxfp4/skinny_table.jsonl
    python scripts/bench_skinny_w4.py --apply profiles/mxfp4/skinny_table.jsonl   # table -> gemm_plan.json "w4plans"
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("qkv_normp", 6144, 4096, 0), ("o_resid", 4096, 4096, 2), ("gate_up_swiglu_normp", 28672, 4096, 1),
          ("down_resid", 4096, 14336, 2)]
MS = [2, 3, 4, 5, 8, 16, 24, 32, 40, 48, 64]
SPLITS = (1, 2, 4, 7, 8)
COLD_BYTES, MIN_LAUNCHES, MARGIN = 600e6, 40, 0.03


def wins(rec) -> bool:
    """The routing rule on one table record."""
    w4, b16 = rec["w4_us"], rec["bf16_routed_us"]
    gap = b16 - w4
    spread = (rec["w4_spread_us"][1] - rec["w4_spread_us"][0]) + (rec["bf16_spread_us"][1] - rec["bf16_spread_us"][0])
    return w4 < (1 - MARGIN) * b16 and gap > spread


def apply(table: str) -> None:
    """gemm_plan.json "w4plans" from the table: per (N, K, mode) a row [M, cfg, split-K] where the W4 kernel won and
    [M, -1, 1] where it lost below a winning M (a row decides (previous M, M]); shapes without a win get no rows."""
    from chronos.ops import gemm

    plan_path = os.path.join(os.path.dirname(os.path.abspath(gemm.__file__)), "gemm_plan.json")
    recs = [json.loads(line) for line in open(table) if line.strip()]
    out = {}
    for r in recs:
        out.setdefault(f"{r['N']},{r['K']},{r['mode']}", []).append(
            [r["M"], r["w4_cfg"], r["w4_splitk"]] if wins(r) else [r["M"], -1, 1])
    w4plans = {}
    for key, rows in out.items():
        rows.sort()
        while rows and rows[-1][1] < 0:  # losses above the last win: no row needed, the last row must be a win
            rows.pop()
        if rows:
            # above the last winning M nothing was measured faster: close the range with the copy
            last = max(r["M"] for r in recs if f"{r['N']},{r['K']},{r['mode']}" == key)
            if rows[-1][0] < last:
                rows.append([last, -1, 1])
            w4plans[key] = rows
    with open(plan_path) as fh:
        plan = json.load(fh)
    plan["w4plans"] = w4plans
    with open(plan_path, "w") as fh:
        json.dump(plan, fh, indent=1)
        fh.write("\n")
    print(json.dumps(w4plans))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--apply", default=None, metavar="TABLE")
    ap.add_argument("--ms", type=int, nargs="*", default=MS)
    ap.add_argument("--kinds", nargs="*", default=[s[0] for s in SHAPES])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--top", type=int, default=3)
    a = ap.parse_args()
    if a.apply:
        return apply(a.apply)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_skinny_w4.py measures GPU kernels: no GPU found")
    from chronos import ops
    from chronos.models.llama import quantize_mxfp4
    from chronos.ops import gemm
    from chronos.ops.gemm import LazyNorm

    ops.load()
    k_ = torch.ops.chronos
    dev, bf = "cuda", torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(0)
    recs = []

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
        n16, n4 = max(c16, MIN_LAUNCHES), max(c4, MIN_LAUNCHES)
        ones = torch.ones(k, device=dev, dtype=bf)
        for m in a.ms:
            s = (torch.randn(m, k, device=dev, generator=gen) + 0.1).to(bf)
            sf = s.float()
            part = torch.stack([(sf[:, i::8] ** 2).sum(1) for i in range(8)], 1).contiguous()
            resid = torch.randn(m, n, device=dev, generator=gen).to(bf) if mode == 2 else None
            pin = None if mode == 2 else part

            def w4(cfg, sk):
                return lambda i: k_.gemm_skinny(s, q4[i % c4][0], mode, cfg, sk, resid, pin, 1e-5, q4[i % c4][1])

            if mode == 2:
                routed = lambda i: ops.gemv_resid(s, w16[i % c16], resid)  # noqa: E731
            elif mode == 1:
                routed = lambda i: ops.gate_up_silu(LazyNorm(s, part, ones, 1e-5), w16[i % c16])  # noqa: E731
            else:
                routed = lambda i: ops.linear(LazyNorm(s, part, ones, 1e-5), w16[i % c16])  # noqa: E731
            bplan = gemm.pp_plan(m, n, k, mode)
            screen = {}
            for cfg in sorted(gemm._SK4):
                for sk in SPLITS:
                    if gemm._sk4_valid(cfg, m, n, k, mode, sk):
                        g = captured(w4(cfg, sk), n4)
                        screen[(cfg, sk)] = replayed(g, n4)
                        del g
            finalists = sorted(screen, key=screen.get)[:a.top]
            gb = captured(routed, n16)
            gs = {c: captured(w4(*c), n4) for c in finalists}
            t, te = {c: [] for c in finalists}, {c: [] for c in finalists}
            tb, tbe = [], []
            for _ in range(a.repeats):  # interleaved: one pass of each in turn, replayed and eager
                tb.append(replayed(gb, n16))
                tbe.append(timed(routed, n16))
                for c in finalists:
                    t[c].append(replayed(gs[c], n4))
                    te[c].append(timed(w4(*c), n4))
            del gb, gs
            best = min(finalists, key=lambda c: statistics.median(t[c]))
            med4, med16 = statistics.median(t[best]), statistics.median(tb)
            rec = dict(kind=kind, N=n, K=k, mode=mode, normp=mode != 2, M=m, copies_bf16=c16, copies_w4=c4,
                       repeats=a.repeats, timing="graph replay", w4_eager_us=round(statistics.median(te[best]), 2),
                       bf16_eager_us=round(statistics.median(tbe), 2), bf16_plan=list(bplan) if bplan else None,
                       bf16_routed_us=round(med16, 2), bf16_spread_us=[round(min(tb), 2), round(max(tb), 2)],
                       w4_cfg=best[0], w4_splitk=best[1], w4_us=round(med4, 2),
                       w4_spread_us=[round(min(t[best]), 2), round(max(t[best]), 2)],
                       w4_tbps=round(b4 / med4 / 1e6, 3), bf16_tbps=round(b16 / med16 / 1e6, 3),
                       speedup=round(med16 / med4, 3),
                       finalists={f"{c[0]}/{c[1]}": round(statistics.median(v), 2) for c, v in t.items()},
                       screen_us={f"{c[0]}/{c[1]}": round(v, 2) for c, v in screen.items()})
            rec["w4_wins"] = wins(rec)
            recs.append(rec)
            print(json.dumps(rec), flush=True)
        del w16, q4
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in recs:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
