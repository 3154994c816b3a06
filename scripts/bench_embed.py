"""Embedding throughput of the engine and the cost of the pooling kernel (csrc/kernels/pool.hip).

Engine part: the 1024 synthetic sensor prompts of the headline wave (bench.py: ``synthetic_chains`` through
``build_prompt``), embedded as raw prompts in one wave per pooling mode with the prefix cache cleared in front of every
wave, as bench.py clears it: embeds/s, prompt tokens/s and the prefix-hit fraction.  ``mean`` takes no prefix hit by
construction; ``last`` shares the template head within the wave.  One warm-up wave per mode on other prompts, then
``--waves`` timed ones; the host clock stops after a device synchronise.

Kernel part: ``ops.pool_accum`` at T = 16384 and T = 1024 rows of H = 4096 (one range per 64 rows into 256 accumulator
rows) next to ``ops.rmsnorm`` on the same rows, which reads the same bytes and writes them back.  One process, the two
kernels in alternating passes, device events around ``LAUNCHES`` back-to-back launches, ``REPEATS`` passes: median and
min..max, warm (the same buffer every launch: at T = 1024 its 8 MiB stay in the caches) and cold (a ring of buffers
larger than the 256 MiB of MALL, so every launch reads HBM).

    python scripts/bench_embed.py [--out profiles/embed/bench_embed.jsonl] [--model llama3-8b] [--waves 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H = 4096
LAUNCHES, REPEATS = 20, 7


def kernel_cost(ops) -> list:
    recs = []
    g = torch.Generator(device="cuda").manual_seed(0)
    for T in (16384, 1024):
        nbuf = max(2, (384 << 20) // (T * H * 2))  # > 256 MiB in flight: every cold launch comes from HBM
        bufs = [(torch.randn(T, H, device="cuda", generator=g)).to(torch.bfloat16) for _ in range(nbuf)]
        B = T // 64
        q = torch.tensor([(64 * b, 64 * b + 64) for b in range(B)], dtype=torch.int32, device="cuda")
        sel = torch.arange(B, dtype=torch.int32, device="cuda")
        acc = torch.zeros(256, H, dtype=torch.float32, device="cuda")
        w = torch.ones(H, dtype=torch.bfloat16, device="cuda")
        fns = {"pool_accum": lambda x: ops.pool_accum(x, 1e-5, q, sel, acc), "rmsnorm": lambda x: ops.rmsnorm(x, w, 1e-5)}
        times = {(k, m): [] for k in fns for m in ("warm", "cold")}
        for fn in fns.values():
            for x in bufs[:2]:
                fn(x)
        torch.cuda.synchronize()
        for _ in range(REPEATS):  # interleaved passes: kernel A warm, B warm, A cold, B cold
            for mode in ("warm", "cold"):
                for name, fn in fns.items():
                    fn(bufs[0])
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(LAUNCHES):
                        fn(bufs[0] if mode == "warm" else bufs[i % nbuf])
                    e1.record()
                    e1.synchronize()
                    times[(name, mode)].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
        for (name, mode), v in times.items():
            rd = T * H * 2
            moved = rd * (2 if name == "rmsnorm" else 1)
            med = statistics.median(v)
            recs.append({"kernel": name, "T": T, "H": H, "cache": mode, "us_median": round(med, 2),
                         "us_min": round(min(v), 2), "us_max": round(max(v), 2), "launches": LAUNCHES,
                         "repeats": REPEATS, "bytes_moved": moved, "GBps": round(moved / med / 1e3, 1)})
        del bufs
    return recs


def engine_waves(a) -> list:
    from chronos.brain.engine.engine import Engine, EngineConfig
    from chronos.sensor.prompt import build_prompt
    from chronos.sensor.replay import synthetic_chains

    eng = Engine(EngineConfig(model=a.model, device="cuda", max_slots=a.streams, max_model_len=512, seed=0,
                              warm_formats=()))
    prompts = [build_prompt(c.history) for c in synthetic_chains(a.streams * (a.waves + 1), seed=1000)]
    recs = []
    for mode in ("mean", "last"):
        for wv in range(a.waves + 1):  # wave 0 warms the mode up
            batch = prompts[wv * a.streams:(wv + 1) * a.streams]
            eng.blocks.clear_cache()
            torch.cuda.synchronize()
            h0, p0 = eng.stats["prefix_hit_tokens"], eng.stats["prefill_steps"]
            t0 = time.perf_counter()
            reqs = [eng.submit_embed(p, pooling=mode) for p in batch]
            eng.run_until_idle()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert all(r.done_reason == "embed" for r in reqs), [r.error for r in reqs if r.error][:3]
            if wv == 0:
                continue
            toks = sum(len(r.prompt_ids) for r in reqs)
            recs.append({"engine": a.model, "pooling": mode, "wave": wv, "embeds": len(reqs), "seconds": round(dt, 4),
                         "embeds_per_s": round(len(reqs) / dt, 1), "prompt_tokens": toks,
                         "tokens_per_s": round(toks / dt, 1),
                         "prefix_hit_fraction": round((eng.stats["prefix_hit_tokens"] - h0) / toks, 4),
                         "prefill_steps": eng.stats["prefill_steps"] - p0})
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--waves", type=int, default=2)
    ap.add_argument("--no-engine", action="store_true", help="kernel timings only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_embed.py measures on the GPU: no GPU found")
    from chronos import ops

    ops.load()
    recs = kernel_cost(ops)
    if not a.no_engine:
        recs += engine_waves(a)
    line = json.dumps({"bench": "embed", "device": torch.cuda.get_device_name(0), "results": recs})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
