"""The W4A16 decode GEMV (csrc/kernels/gemv.hip W4: OCP MXFP4 weights) against the bf16 kernels on the dequantised copy
of the same weights, per Llama-3-8B projection and M = 1, 2, 4.

One process, the candidates interleaved.  Per shape: QKV + RoPE + paged-KV write, the O residual producer, gate_up
with SwiGLU and the folded norm (NORMP), the down residual producer — the fused forms at M <= 2, the plain / SwiGLU
GEMV at M = 4 (the fused epilogues take two rows).  Three candidates:

* ``w4``:          the fp4 GEMV kernel;
* ``bf16_gemv``:   the bf16 GEMV kernel on ``.w`` (the same epilogue);
* ``bf16_routed``: what ``chronos.ops`` runs on ``.w`` for the plain / SwiGLU form at this M (the skinny MFMA GEMM
                   above GEMV_MAX_M) — what the model would run instead of the fp4 kernel.

Weights are cold: every launch takes the next of enough copies to exceed 600 MB (the MALL is 256 MB), as the plan
tuner does.  Device events around one pass over the copies (at least 40 launches), median of 7 interleaved repeats
after a warm-up pass.  Reports us per launch and weight TB/s (bf16: 2 N K bytes; mxfp4: N K / 2 + N K / 32).
``--sweep`` adds the fp4 kernel's rows-per-group knobs at M = 1.

    python scripts/bench_gemv_w4.py [--out profiles/mxfp4/gemv_table.jsonl] [--sweep]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("qkv_rope", 6144, 4096), ("o_resid", 4096, 4096), ("gate_up_swiglu_normp", 28672, 4096),
          ("down_resid", 4096, 14336)]
REPEATS, COLD_BYTES, MIN_LAUNCHES = 7, 600e6, 40
SWEEP = {"qkv_rope": ("gemv_w4_r_rope", (2, 4, 8)), "o_resid": ("gemv_w4_r_resid", (2, 4, 8)),
         "gate_up_swiglu_normp": ("gemv_w4_r_swiglu", (1, 2, 4, 8)), "down_resid": ("gemv_w4_r_resid", (2, 4, 8))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 2, 4])
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemv_w4.py measures GPU kernels: no GPU found")
    from chronos import ops
    from chronos.models.llama import LlamaConfig, Q4Tensor, quantize_mxfp4, rope_table

    ops.load()
    k_ = torch.ops.chronos
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    bf = torch.bfloat16
    hq, hkv = 32, 8
    cs = rope_table(LlamaConfig(name="t"), 4096, dev)
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

    for kind, n, k in SHAPES:
        w0 = quantize_mxfp4((torch.randn(n, k, device=dev, generator=gen) * 0.02).to(bf))
        b16, b4 = 2 * n * k, n * k // 2 + n * k // 32
        c16 = max(2, int(-(-COLD_BYTES // b16)))
        c4 = max(2, int(-(-COLD_BYTES // b4)))
        w16 = [w0.w.clone() for _ in range(c16)]
        w4 = [Q4Tensor(w0.q.clone(), w0.e.clone(), w16[0]) for _ in range(c4)]
        for m in a.rows:
            x = (torch.randn(m, k, device=dev, generator=gen) + 0.1).to(bf)
            fused = m <= 2
            swiglu = kind.startswith("gate_up")
            cands = {}
            if kind == "qkv_rope" and fused:
                kc = torch.zeros(64, hkv, 16, 128, device=dev, dtype=bf)
                vc = torch.zeros(64, hkv, 128, 16, device=dev, dtype=bf)
                bt = torch.arange(1, 1 + 4 * m, device=dev, dtype=torch.int32).view(m, 4)
                pos = torch.tensor([37, 50][:m], device=dev, dtype=torch.int32)
                ts = torch.arange(m, device=dev, dtype=torch.int32)
                q = torch.zeros(m, hq, 128, device=dev, dtype=bf)
                rope = lambda w, we: k_.qkv_rope(x, None, 0.0, w, pos, ts, bt, cs, q, kc, vc, hq, hkv, 1.0, 1.0,  # noqa: E731
                                                 None, we)
                cands["w4"] = lambda i: rope(w4[i % c4].q, w4[i % c4].e)
                cands["bf16_gemv"] = lambda i: rope(w16[i % c16], None)
            elif kind.endswith("resid") and fused:
                r = torch.randn(m, n, device=dev, generator=gen).to(bf)
                s = torch.empty_like(r)
                cands["w4"] = lambda i: k_.gemv_resid(x, w4[i % c4].q, r, s, None, w4[i % c4].e)
                cands["bf16_gemv"] = lambda i: k_.gemv_resid(x, w16[i % c16], r, s)
            elif swiglu and fused:
                # the producer's residual stream and partials (a K x K residual GEMV), consumed through NORMP
                wo = (torch.randn(k, k, device=dev, generator=gen) * 0.02).to(bf)
                r = torch.randn(m, k, device=dev, generator=gen).to(bf)
                s = torch.empty_like(r)
                part = k_.gemv_resid(x, wo, r, s)
                cands["w4"] = lambda i: k_.gemv_normp(s, part, 1e-5, w4[i % c4].q, True, None, w4[i % c4].e)
                cands["bf16_gemv"] = lambda i: k_.gemv_normp(s, part, 1e-5, w16[i % c16], True)
            else:
                cands["w4"] = lambda i: k_.gemv(x, w4[i % c4].q, swiglu, None, w4[i % c4].e)
                cands["bf16_gemv"] = lambda i: k_.gemv(x, w16[i % c16], swiglu)
            # what chronos.ops runs on the bf16 copy for the plain / SwiGLU form at this M
            cands["bf16_routed"] = (lambda i: ops.gate_up_silu(x, w16[i % c16])) if swiglu else \
                (lambda i: ops.linear(x, w16[i % c16]))
            nl = {"w4": max(c4, MIN_LAUNCHES), "bf16_gemv": max(c16, MIN_LAUNCHES), "bf16_routed": max(c16, MIN_LAUNCHES)}

            def measure(cs_):
                for name, fn in cs_.items():
                    timed(fn, nl.get(name, max(c4, MIN_LAUNCHES)))  # warm-up: code objects, allocator
                t = {name: [] for name in cs_}
                for _ in range(REPEATS):
                    for name, fn in cs_.items():  # interleaved: one repeat of each in turn
                        t[name].append(timed(fn, nl.get(name, max(c4, MIN_LAUNCHES))))
                return t

            t = measure(cands)
            med = {name: statistics.median(v) for name, v in t.items()}
            best16 = min(med["bf16_gemv"], med["bf16_routed"]) if not fused else med["bf16_gemv"]
            rec = dict(kind=kind, fused_epilogue=fused, N=n, K=k, M=m, copies_bf16=c16, copies_w4=c4, repeats=REPEATS,
                       w4_us=round(med["w4"], 2), bf16_gemv_us=round(med["bf16_gemv"], 2),
                       bf16_routed_us=round(med["bf16_routed"], 2),
                       w4_tbps=round(b4 / med["w4"] / 1e6, 3), bf16_gemv_tbps=round(b16 / med["bf16_gemv"] / 1e6, 3),
                       bf16_routed_tbps=round(b16 / med["bf16_routed"] / 1e6, 3),
                       speedup_vs_bf16=round(best16 / med["w4"], 3), w4_wins=bool(med["w4"] < best16),
                       spread_us={name: [round(min(v), 2), round(max(v), 2)] for name, v in t.items()})
            recs.append(rec)
            print(json.dumps(rec), flush=True)
            if a.sweep and m == 1:
                knob, vals = SWEEP[kind]
                sw = {}
                for v in vals:
                    k_.set_knob(knob, v)
                    try:
                        tt = measure({"w4": cands["w4"]})
                    finally:
                        k_.set_knob(knob, -1)
                    sw[str(v)] = round(statistics.median(tt["w4"]), 2)
                rec = dict(kind=kind, N=n, K=k, M=1, sweep_knob=knob, w4_us_by_rows=sw)
                recs.append(rec)
                print(json.dumps(rec), flush=True)
        del w16, w4
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in recs:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
