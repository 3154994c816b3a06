"""Cost of the min_p / typical_p kernel (csrc/kernels/truncate.hip) next to the sampler launch it precedes, on the
Llama-3 vocabulary width.

One process, the two kernels interleaved: truncate_logits and constrained_sample (temperature 1, no top-k / top-p: the
one-pass Gumbel arg-max a truncating request takes afterwards) on the same bf16 logits, at 1 row (single stream) and
1024 rows (the wave), in the free grammar's start state (every token of the text vocabulary legal) and in the verdict
schema's start state (a handful of legal tokens: both kernels still walk the whole DFA row), with min_p only (0.05),
typical_p only (0.9) and both.  Every launch starts from the same slot state and the same logits: a few tiny device
copies restore the state and one device copy restores the logits the truncation rewrote; the same copies precede
every timed launch of either kernel, and their own cost is measured and subtracted.  Device events around 50 launches,
median of 7 repeats after a warm-up.

    python scripts/bench_truncate.py [--out profiles/truncate/kernel_cost.jsonl]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 128256
LAUNCHES, REPEATS, MAX_OUT = 50, 7, 64
MODES = {"min_p": (0.05, 1.0), "typical_p": (0.0, 0.9), "both": (0.05, 0.9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 1024])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_truncate.py measures GPU kernels: no GPU found")
    from chronos import ops
    from chronos.brain.constrain import DONE, GrammarBank
    from chronos.brain.tokenizer import load_tokenizer
    from chronos.sensor.prompt import VERDICT_SCHEMA

    ops.load()
    tok = load_tokenizer(None)
    bank = GrammarBank(tok.token_bytes_list(), tok.stop_ids, V, 1024, "cuda")
    starts = {"free": bank.get(None).start, "verdict": bank.get(VERDICT_SCHEMA).start}
    i32 = dict(dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    recs = []
    for rows in a.rows:
        logits0 = (torch.randn(rows, V, device="cuda", generator=gen) * 2.0).to(torch.bfloat16)
        logits = logits0.clone()
        for gname, start in starts.items():
            nx = bank.next[start].long()
            legal = int(((nx >= 0) & (bank.dist[nx.clamp(min=0)] <= 59)).sum())
            for mode, (minp, typ) in MODES.items():
                st0, rem0, nout0 = torch.full((rows,), start, **i32), torch.full((rows,), 60, **i32), \
                    torch.zeros(rows, **i32)
                st, rem, nout = st0.clone(), rem0.clone(), nout0.clone()
                z = [torch.zeros(rows, **i32) for _ in range(3)]
                outt = torch.zeros(rows, MAX_OUT, **i32)
                temp = torch.ones(rows, device="cuda")
                seed = torch.arange(rows, **i32)
                lnp = torch.full((rows,), math.log(minp) if minp > 0 else -math.inf, device="cuda")
                tp = torch.full((rows,), typ, device="cuda")

                def restore():
                    st.copy_(st0)
                    rem.copy_(rem0)
                    nout.copy_(nout0)
                    logits.copy_(logits0)

                def truncate():
                    ops.truncate_logits(logits, None, bank.next, bank.dist, DONE, st, rem, temp, lnp, tp)

                def sample():
                    ops.constrained_sample(logits, None, bank.next, bank.dist, DONE, st, rem, temp, seed, z[0], z[1],
                                           z[2], nout, outt)

                fns = {"restore": lambda: None, "truncate_logits": truncate, "constrained_sample": sample}

                def timed(fn):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(LAUNCHES):
                        restore()
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1) / LAUNCHES * 1e3

                restore(); truncate(); sample()  # noqa: E702 — warm-up (code objects)
                kept = int((logits[0, :bank.next.shape[1]].float() > -math.inf).sum())
                ts = {k: [] for k in fns}
                for _ in range(REPEATS):
                    for k, fn in fns.items():  # interleaved: one repeat of each in turn
                        ts[k].append(timed(fn))
                med = {k: statistics.median(v) for k, v in ts.items()}
                base = med["restore"]
                tr_us, smp_us = med["truncate_logits"] - base, med["constrained_sample"] - base
                rec = dict(rows=rows, vocab=V, grammar=gname, legal_tokens=legal, mode=mode, min_p=minp,
                           typical_p=typ, finite_logits_row0_after=kept, launches=LAUNCHES, repeats=REPEATS,
                           restore_overhead_us=round(base, 2), truncate_logits_us=round(tr_us, 2),
                           constrained_sample_us=round(smp_us, 2), truncate_over_sampler=round(tr_us / smp_us, 3),
                           spread_us={k: [round(min(v), 2), round(max(v), 2)] for k, v in ts.items()})
                recs.append(rec)
                print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in recs:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
