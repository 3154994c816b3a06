"""Cost of the repeat / frequency / presence penalty kernel (csrc/kernels/penalties.hip) next to the sampler launch it
precedes, on the Llama-3 vocabulary width.

One process, the two kernels interleaved: apply_penalties and constrained_sample (greedy, free grammar) on the same
bf16 logits, at 1 row (single stream) and 1024 rows (the wave), with a history window of L = 64 and L = 1024 ids (every
row's window full: a full prompt tail of random ids, so nearly all of them are distinct and each costs one logit
read-modify-write).  Every launch starts from the same slot state (a few tiny device copies restore it; the same
copies precede every timed launch and their own cost is measured and subtracted), device events around 50 launches,
median of 7 repeats after a warm-up.  The penalty kernel rewrites its L logits per row in place at every launch, so
their values drift over the run (repeat_penalty 1.1 only: towards 0 and -inf); neither kernel's greedy path depends on
the values, and the logits are drawn afresh for every configuration.

    python scripts/bench_penalties.py [--out profiles/penalties/kernel_cost.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 128256
LAUNCHES, REPEATS, MAX_OUT = 50, 7, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 1024])
    ap.add_argument("--windows", type=int, nargs="*", default=[64, 1024])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_penalties.py measures GPU kernels: no GPU found")
    from chronos import ops
    from chronos.brain.constrain import DONE, GrammarBank
    from chronos.brain.tokenizer import load_tokenizer

    ops.load()
    tok = load_tokenizer(None)
    bank = GrammarBank(tok.token_bytes_list(), tok.stop_ids, V, 1024, "cuda")
    start = bank.get(None).start
    i32 = dict(dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    recs = []
    for rows in a.rows:
        for L in a.windows:
            logits = torch.randn(rows, V, device="cuda", generator=gen).to(torch.bfloat16)
            st0, rem0, nout0 = torch.full((rows,), start, **i32), torch.full((rows,), 60, **i32), \
                torch.zeros(rows, **i32)
            st, rem, nout = st0.clone(), rem0.clone(), nout0.clone()
            z = [torch.zeros(rows, **i32) for _ in range(3)]
            outt = torch.zeros(rows, MAX_OUT, **i32)
            par = torch.tensor([1.1, 0.0, 0.0], device="cuda").repeat(rows, 1)
            last = torch.full((rows,), L, **i32)
            tail = torch.randint(0, V, (rows, L), generator=gen, **i32)
            tlen = torch.full((rows,), L, **i32)

            def restore():
                st.copy_(st0)
                rem.copy_(rem0)
                nout.copy_(nout0)

            def penalties():
                ops.apply_penalties(logits, None, DONE, st, nout, outt, par, last, tail, tlen)

            def sample():
                ops.constrained_sample(logits, None, bank.next, bank.dist, DONE, st, rem, None, None, z[0], z[1], z[2],
                                       nout, outt)

            fns = {"restore": lambda: None, "apply_penalties": penalties, "constrained_sample": sample}

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

            restore(); penalties(); sample()  # noqa: E702 — warm-up (code objects)
            ts = {k: [] for k in fns}
            for _ in range(REPEATS):
                for k, fn in fns.items():  # interleaved: one repeat of each in turn
                    ts[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in ts.items()}
            base = med["restore"]
            pen_us, smp_us = med["apply_penalties"] - base, med["constrained_sample"] - base
            rec = dict(rows=rows, vocab=V, window=L, launches=LAUNCHES, repeats=REPEATS,
                       distinct_ids_row0=int(torch.unique(tail[0]).numel()),
                       restore_overhead_us=round(base, 2), apply_penalties_us=round(pen_us, 2),
                       constrained_sample_us=round(smp_us, 2), penalties_over_sampler=round(pen_us / smp_us, 3),
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
