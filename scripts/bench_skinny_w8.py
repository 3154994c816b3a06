"""The W8A16 mode of the skinny MFMA GEMM (csrc/kernels/gemm_skinny.hip WM = kW8: e4m3 weights with per-row scales, bf16
activations) against what an fp8 model runs today at the same rows, per Llama-3-8B projection at M = 2 .. 64.

One process.  Per projection the epilogue the model uses in a W8A16 step: QKV plain with the folded norm (NORMP), O and
down the residual producer (kResid), gate_up SwiGLU + NORMP.  Candidates:

* every valid W8 config x split-K (``ops/gemm.py`` ``_SK8`` / ``_sk8_valid``), screened with one timed pass each; the
  ``--top`` fastest go on to the repeats;
* ``today``: the W8A8 op ``ops.qlinear`` on quantised activations — alone (``qlinear_us``: the comparison the routing
  rule uses, the one less favourable to the new kernel, since the W8A8 path also pays for its quantisation) and with
  the ``ops.quant_rows`` launch in front of it (``quant_qlinear_us``).  At M = 2 today's route is the W8A16 GEMV
  (``ops.linear`` / ``ops.gate_up_silu`` on the QTensor with the model's LazyNorm input; O and down: the plain GEMV);
* ``bf16_skinny``: the routed bf16 kernel on the unquantised weight, the yardstick on twice the bytes.

Weights are cold: every launch takes the next of enough copies to exceed 600 MB (the MALL is 256 MB).  A pass is one
launch per copy (at least 40 launches) between two device events, and every pass is the replay of a captured graph of
those launches, so the figures are kernel times.  Finalists, today's route and the yardstick are interleaved for
``--repeats`` passes; reported are the medians and the [min, max] of the passes, and TB/s of each kernel's own weight
bytes.  ``w8_wins``: the best W8 median is more than 3 % below ``qlinear_us`` (M = 2: the GEMV) and the gap is larger
than both spreads together.

    python scripts/bench_skinny_w8.py --out profiles/fp8/skinny_table.jsonl
    python scripts/bench_skinny_w8.py --apply profiles/fp8/skinny_table.jsonl   # table -> gemm_plan.json "w8plans"
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("qkv_normp", 6144, 4096, 0), ("o_resid", 4096, 4096, 2), ("gate_up_swiglu_normp", 28672, 4096, 1),
          ("down_resid", 4096, 14336, 2)]
MS = [2, 3, 4, 8, 16, 24, 32, 40, 48, 64]
SPLITS = (1, 2, 4, 7, 8)
COLD_BYTES, MIN_LAUNCHES, MARGIN = 600e6, 40, 0.03


def wins(rec) -> bool:
    """The routing rule on one table record."""
    w8, ref = rec["w8_us"], rec["today_us"]
    spread = (rec["w8_spread_us"][1] - rec["w8_spread_us"][0]) + (rec["today_spread_us"][1] - rec["today_spread_us"][0])
    return w8 < (1 - MARGIN) * ref and ref - w8 > spread


def apply(table: str) -> None:
    """gemm_plan.json "w8plans" from the table: per (N, K, mode) a row [M, cfg, split-K] where the W8 kernel won and
    [M, -1, 1], a recorded loss, where it did not."""
    from chronos.ops import gemm

    plan_path = os.path.join(os.path.dirname(os.path.abspath(gemm.__file__)), "gemm_plan.json")
    recs = [json.loads(line) for line in open(table) if line.strip()]
    w8plans = {}
    for r in recs:
        w8plans.setdefault(f"{r['N']},{r['K']},{r['mode']}", []).append(
            [r["M"], r["w8_cfg"], r["w8_splitk"]] if wins(r) else [r["M"], -1, 1])
    for rows in w8plans.values():
        rows.sort()
    with open(plan_path) as fh:
        plan = json.load(fh)
    plan["w8plans"] = w8plans
    with open(plan_path, "w") as fh:
        json.dump(plan, fh, indent=1)
        fh.write("\n")
    print(json.dumps(w8plans))


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
        raise SystemExit("bench_skinny_w8.py measures GPU kernels: no GPU found")
    from chronos import ops
    from chronos.models.llama import QTensor
    from chronos.ops import gemm
    from chronos.ops import reference as ref
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
        w = (torch.randn(n, k, device=dev, generator=gen) * 0.02).to(bf)
        wq, ws = ref.quantize_weight(w)
        wq, ws = wq.contiguous(), ws.contiguous()
        b16, b8 = 2 * n * k, n * k + 4 * n
        c16 = max(2, int(-(-COLD_BYTES // b16)))
        c8 = max(2, int(-(-COLD_BYTES // b8)))
        w16 = [w.clone() for _ in range(c16)]
        q8 = [QTensor(wq.clone(), ws.clone()) for _ in range(c8)]
        n16, n8 = max(c16, MIN_LAUNCHES), max(c8, MIN_LAUNCHES)
        ones = torch.ones(k, device=dev, dtype=bf)
        for m in a.ms:
            s = (torch.randn(m, k, device=dev, generator=gen) + 0.1).to(bf)
            sf = s.float()
            part = torch.stack([(sf[:, i::8] ** 2).sum(1) for i in range(8)], 1).contiguous()
            resid = torch.randn(m, n, device=dev, generator=gen).to(bf) if mode == 2 else None
            pin = None if mode == 2 else part
            xq, xs = ops.quant_rows(s)

            def w8(cfg, sk):
                return lambda i: k_.gemm_skinny(s, q8[i % c8].q, mode, cfg, sk, resid, pin, 1e-5, None, q8[i % c8].s)

            def on(ws_, lazy=True):
                x = (lambda: LazyNorm(s, part, ones, 1e-5)) if lazy and mode != 2 else (lambda: s)
                if mode == 2:
                    return lambda i: ops.gemv_resid(x(), ws_[i % len(ws_)], resid)
                if mode == 1:
                    return lambda i: ops.gate_up_silu(x(), ws_[i % len(ws_)])
                return lambda i: ops.linear(x(), ws_[i % len(ws_)])

            qlin = lambda i: ops.qlinear(xq, xs, q8[i % c8].q, q8[i % c8].s, mode == 1)  # noqa: E731
            quant_qlin = lambda i: ops.qlinear(*ops.quant_rows(s), q8[i % c8].q, q8[i % c8].s, mode == 1)  # noqa: E731
            # M <= 2: the W8A16 GEMV — its residual producer where that takes the rows, else (O / down at M = 2) the plain
            # GEMV, whose separate residual add + norm launch is left out: the comparison less favourable to the new kernel
            gemv = m <= 2 and ops.gemv_q_ok(m, n, k)
            if gemv and mode == 2 and not ops.resid_ok(m, n, k, True):
                today = lambda i: ops.linear(s, q8[i % c8])  # noqa: E731
            else:
                today = on(q8) if gemv else qlin
            bplan = gemm.pp_plan(m, n, k, mode)
            screen = {}
            for cfg in sorted(gemm._SK8):
                for sk in SPLITS:
                    if gemm._sk8_valid(cfg, m, n, k, mode, sk):
                        g = captured(w8(cfg, sk), n8)
                        screen[(cfg, sk)] = replayed(g, n8)
                        del g
            finalists = sorted(screen, key=screen.get)[:a.top]
            gt, gq = captured(today, n8), captured(quant_qlin, n8)
            gb = captured(on(w16), n16) if (bplan is not None or m <= gemm.GEMV_MAX_M) else None
            gs = {c: captured(w8(*c), n8) for c in finalists}
            t = {c: [] for c in finalists}
            tt, tq, tb = [], [], []
            for _ in range(a.repeats):  # interleaved: one pass of each in turn
                tt.append(replayed(gt, n8))
                tq.append(replayed(gq, n8))
                if gb is not None:
                    tb.append(replayed(gb, n16))
                for c in finalists:
                    t[c].append(replayed(gs[c], n8))
            del gt, gq, gb, gs
            best = min(finalists, key=lambda c: statistics.median(t[c]))
            med8, medt, medq = statistics.median(t[best]), statistics.median(tt), statistics.median(tq)
            medb = statistics.median(tb) if tb else None
            rec = dict(kind=kind, N=n, K=k, mode=mode, normp=mode != 2, M=m, copies_bf16=c16, copies_w8=c8,
                       repeats=a.repeats, timing="graph replay", today="w8a16_gemv" if gemv else "qlinear",
                       today_us=round(medt, 2), today_spread_us=[round(min(tt), 2), round(max(tt), 2)],
                       quant_qlinear_us=round(medq, 2), quant_qlinear_spread_us=[round(min(tq), 2), round(max(tq), 2)],
                       bf16_plan=list(bplan) if bplan else None, bf16_skinny_us=round(medb, 2) if medb else None,
                       bf16_spread_us=[round(min(tb), 2), round(max(tb), 2)] if tb else None,
                       w8_cfg=best[0], w8_splitk=best[1], w8_us=round(med8, 2),
                       w8_spread_us=[round(min(t[best]), 2), round(max(t[best]), 2)],
                       w8_tbps=round(b8 / med8 / 1e6, 3), today_tbps=round(b8 / medt / 1e6, 3),
                       bf16_tbps=round(b16 / medb / 1e6, 3) if medb else None, speedup=round(medt / med8, 3),
                       speedup_vs_quant_qlinear=round(medq / med8, 3),
                       finalists={f"{c[0]}/{c[1]}": round(statistics.median(v), 2) for c, v in t.items()},
                       screen_us={f"{c[0]}/{c[1]}": round(v, 2) for c, v in screen.items()})
            rec["w8_wins"] = wins(rec)
            recs.append(rec)
            print(json.dumps(rec), flush=True)
            if a.out:  # the table so far, after every point
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as fh:
                    for r in recs:
                        fh.write(json.dumps(r) + "\n")
        del w16, q8
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
