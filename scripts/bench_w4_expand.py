"""The MXFP4 expansion kernel (csrc/kernels/w4_expand.hip) and what the packed-only weight mode pays for it, per
Llama-3-8B projection.  One process, built like scripts/bench_skinny_w4.py: cold weights (every launch takes the next
of enough copies to exceed 600 MB; the MALL is 256 MB), every pass that counts the replay of a captured graph of those
launches between two device events, the alternatives interleaved for ``--repeats`` passes, medians with [min, max].

(a) ``expand``: the expansion alone (q / e -> the one scratch) against a device-to-device ``copy_`` of a bf16 [N, K]
    tensor into one destination.  The copy moves 4 B per element, the expansion 2.53.  ``no_slower`` is the
    requirement: the expansion's median is not above the copy's by more than the copy's own spread.
(b) ``gemm``: what ``chronos.ops`` runs on a packed-only Q4Tensor (the expansion + the routed bf16 GEMM on the scratch)
    against the same call on a resident bf16 copy, with the production epilogues (QKV plain + folded norm, O / down the
    residual producer, gate_up SwiGLU + folded norm) at M = 128, 1024, 4096, 16384.
(c) ``skinny``: QKV and gate_up at M = 40 / 48 / 64, the six points where the W4A16 skinny kernel lost to the resident
    copy: the packed-only route there (the ``_sk4_model`` config of the W4A16 kernel) against the expansion + the bf16
    kernel it is routed instead of, and the resident copy for reference.

    python scripts/bench_w4_expand.py --out profiles/mxfp4/expand_table.jsonl
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("qkv_normp", 6144, 4096, 0), ("o_resid", 4096, 4096, 2), ("gate_up_swiglu_normp", 28672, 4096, 1),
          ("down_resid", 4096, 14336, 2)]
MS = [128, 1024, 4096, 16384]
SKINNY_POINTS = {"qkv_normp": [40, 48, 64], "gate_up_swiglu_normp": [40, 48, 64]}
COLD_BYTES, MIN_LAUNCHES = 600e6, 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ms", type=int, nargs="*", default=MS)
    ap.add_argument("--kinds", nargs="*", default=[s[0] for s in SHAPES])
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_w4_expand.py measures GPU kernels: no GPU found")
    from chronos import ops
    from chronos.models.llama import Q4Tensor, quantize_mxfp4
    from chronos.ops import gemm
    from chronos.ops.gemm import LazyNorm

    ops.load()
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

    def interleaved(alts):
        """alts: name -> (graph, launches).  name -> (median us, [min, max]) over the interleaved repeats."""
        t = {name: [] for name in alts}
        for _ in range(a.repeats):
            for name, (g, n) in alts.items():
                t[name].append(replayed(g, n))
        return {name: (round(statistics.median(v), 2), [round(min(v), 2), round(max(v), 2)]) for name, v in t.items()}

    def emit(rec):
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    for kind, n, k, mode in SHAPES:
        if kind not in a.kinds:
            continue
        w0 = quantize_mxfp4((torch.randn(n, k, device=dev, generator=gen) * 0.02).to(bf))
        b16, b4 = 2 * n * k, n * k // 2 + n * k // 32
        c16 = max(2, int(-(-COLD_BYTES // b16)))
        c4 = max(2, int(-(-COLD_BYTES // b4)))
        w16 = [w0.w.clone() for _ in range(c16)]
        scratch = ops.W4Scratch(n * k, dev)
        q4 = [Q4Tensor(w0.q.clone(), w0.e.clone(), None, scratch) for _ in range(c4)]
        dst = torch.empty(n, k, device=dev, dtype=bf)
        assert torch.equal(ops.w4_dense(q4[0]), w0.w)  # the same bits
        # ---- (a) the expansion against a device-to-device copy ----
        n16, n4 = max(c16, MIN_LAUNCHES), max(c4, MIN_LAUNCHES)
        alts = {"expand": (captured(lambda i: ops.w4_expand(q4[i % c4].q, q4[i % c4].e, scratch.buf), n4), n4),
                "copy": (captured(lambda i: dst.copy_(w16[i % c16]), n16), n16)}
        r = interleaved(alts)
        del alts
        ex, cp = r["expand"], r["copy"]
        emit(dict(part="expand", kind=kind, N=n, K=k, copies_w4=c4, copies_bf16=c16, repeats=a.repeats,
                  timing="graph replay", expand_us=ex[0], expand_spread_us=ex[1], copy_us=cp[0], copy_spread_us=cp[1],
                  expand_tbps=round((b4 + b16) / ex[0] / 1e6, 3), copy_tbps=round(2 * b16 / cp[0] / 1e6, 3),
                  expand_over_copy=round(ex[0] / cp[0], 3), no_slower=bool(ex[0] <= cp[0] + (cp[1][1] - cp[1][0]))))
        ones = torch.ones(k, device=dev, dtype=bf)

        def call(m, weights, nw):
            s = (torch.randn(m, k, device=dev, generator=gen) + 0.1).to(bf)
            sf = s.float()
            part = torch.stack([(sf[:, i::8] ** 2).sum(1) for i in range(8)], 1).contiguous()
            del sf
            if mode == 2:
                resid = torch.randn(m, n, device=dev, generator=gen).to(bf)
                return lambda i: ops.gemv_resid(s, weights[i % nw], resid)
            if mode == 1:
                return lambda i: ops.gate_up_silu(LazyNorm(s, part, ones, 1e-5), weights[i % nw])
            return lambda i: ops.linear(LazyNorm(s, part, ones, 1e-5), weights[i % nw])

        # ---- (b) expansion + routed bf16 GEMM against the GEMM on a resident copy ----
        for m in a.ms:
            nl16, nl4 = (max(c16, MIN_LAUNCHES), max(c4, MIN_LAUNCHES)) if m <= 1024 else (max(c16, 8), max(c4, 8))
            e0 = gemm.w4_stats["expand_launches"]
            alts = {"packed": (captured(call(m, q4, c4), nl4), nl4), "copy": (captured(call(m, w16, c16), nl16), nl16)}
            assert gemm.w4_stats["expand_launches"] - e0 == nl4 + 2  # every packed launch expanded
            r = interleaved(alts)
            del alts
            pk, cp = r["packed"], r["copy"]
            bplan = gemm.pp_plan(m, n, k, mode)
            emit(dict(part="gemm", kind=kind, N=n, K=k, mode=mode, M=m, repeats=a.repeats, timing="graph replay",
                      bf16_plan=list(bplan) if bplan else None, packed_us=pk[0], packed_spread_us=pk[1],
                      copy_us=cp[0], copy_spread_us=cp[1], expand_us=ex[0], packed_over_copy=round(pk[0] / cp[0], 3)))
            torch.cuda.empty_cache()
        # ---- (c) the M = 40 / 48 / 64 points the W4A16 skinny kernel lost to the resident copy ----
        for m in SKINNY_POINTS.get(kind, []):
            nl16, nl4 = max(c16, MIN_LAUNCHES), max(c4, MIN_LAUNCHES)
            assert gemm.w4_plan(m, n, k, mode) is None  # copy mode: the copy
            plan = gemm.w4_plan(m, n, k, mode, packed=True)
            assert plan is not None and plan == gemm._sk4_model(m, n, k, mode)
            s0 = gemm.w4_stats["skinny_launches"]
            g_sk = captured(call(m, q4, c4), nl4)
            assert gemm.w4_stats["skinny_launches"] - s0 == nl4 + 2
            old = gemm.W4_SKINNY
            gemm.W4_SKINNY = "off"  # the route packed-only would take otherwise: expansion + the bf16 kernel
            try:
                e0 = gemm.w4_stats["expand_launches"]
                g_ex = captured(call(m, q4, c4), nl4)
                assert gemm.w4_stats["expand_launches"] - e0 == nl4 + 2
            finally:
                gemm.W4_SKINNY = old
            alts = {"w4_skinny": (g_sk, nl4), "expand_bf16": (g_ex, nl4), "copy": (captured(call(m, w16, c16), nl16), nl16)}
            r = interleaved(alts)
            del alts, g_sk, g_ex
            emit(dict(part="skinny", kind=kind, N=n, K=k, mode=mode, M=m, repeats=a.repeats, timing="graph replay",
                      w4_cfg=plan[0], w4_splitk=plan[1], w4_skinny_us=r["w4_skinny"][0],
                      w4_skinny_spread_us=r["w4_skinny"][1], expand_bf16_us=r["expand_bf16"][0],
                      expand_bf16_spread_us=r["expand_bf16"][1], copy_us=r["copy"][0], copy_spread_us=r["copy"][1],
                      w4_skinny_over_copy=round(r["w4_skinny"][0] / r["copy"][0], 3),
                      expand_bf16_over_w4_skinny=round(r["expand_bf16"][0] / r["w4_skinny"][0], 3)))
        del w16, q4, scratch, dst
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in recs:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
