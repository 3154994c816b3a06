"""Cost of the two Mirostat 2.0 kernels (csrc/kernels/mirostat.hip) next to the sampler launch they bracket, on the
Llama-3 vocabulary width.

One process, the three kernels interleaved: mirostat_truncate, constrained_sample (temperature 1, no top-k / top-p:
the one-pass Gumbel arg-max a mirostat request takes) and mirostat_update on the same bf16 logits, at 1 row (single
stream) and 1024 rows (the wave), in the free grammar's start state (every token of the text vocabulary legal) and in
the verdict schema's start state (a handful of legal tokens: the kernels still walk the whole DFA row), at the default
tau = 5, eta = 0.1 and the starting mu = 2 * tau.  Every launch starts from the same slot state, mu and logits: a few
tiny device copies restore the state and one device copy restores the logits the truncation rewrote; the same copies
precede every timed launch of each kernel, and their own cost is measured and subtracted.  The update kernel is timed
on the state the first two left (mark set, nout advanced by one).  Device events around 50 launches, median of 7
repeats after a warm-up.

    python scripts/bench_mirostat.py [--out profiles/mirostat/kernel_cost.jsonl]
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
TAU, ETA = 5.0, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 1024])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mirostat.py measures GPU kernels: no GPU found")
    from chronos import ops
    from chronos.brain.constrain import DONE, GrammarBank
    from chronos.brain.tokenizer import load_tokenizer
    from chronos.sensor.prompt import VERDICT_SCHEMA

    ops.load()
    tok = load_tokenizer(None)
    bank = GrammarBank(tok.token_bytes_list(), tok.stop_ids, V, 1024, "cuda")
    starts = {"free": bank.get(None).start, "verdict": bank.get(VERDICT_SCHEMA).start}
    i32 = dict(dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    recs = []
    for rows in a.rows:
        logits0 = (torch.randn(rows, V, device="cuda", generator=gen) * 2.0).to(torch.bfloat16)
        logits = logits0.clone()
        for gname, start in starts.items():
            nx = bank.next[start].long()
            legal = int(((nx >= 0) & (bank.dist[nx.clamp(min=0)] <= 59)).sum())
            st0, rem0, nout0 = torch.full((rows,), start, **i32), torch.full((rows,), 60, **i32), \
                torch.zeros(rows, **i32)
            st, rem, nout = st0.clone(), rem0.clone(), nout0.clone()
            z = [torch.zeros(rows, **i32) for _ in range(3)]
            outt = torch.zeros(rows, MAX_OUT, **i32)
            temp = torch.ones(rows, device="cuda")
            seed = torch.arange(rows, **i32)
            on = torch.ones(rows, **i32)
            mu0 = torch.full((rows,), 2 * TAU, **f32)
            mu, tau, eta = mu0.clone(), torch.full((rows,), TAU, **f32), torch.full((rows,), ETA, **f32)
            m, lnz, mark = torch.zeros(rows, **f32), torch.zeros(rows, **f32), torch.full((rows,), -1, **i32)
            nout1 = nout0 + 1  # what the sampler leaves: the update kernel's "advanced past the mark"

            def restore():
                st.copy_(st0)
                rem.copy_(rem0)
                nout.copy_(nout0)
                mu.copy_(mu0)
                logits.copy_(logits0)

            def truncate():
                ops.mirostat_truncate(logits, None, bank.next, bank.dist, DONE, st, rem, nout, temp, on, mu, m, lnz,
                                      mark)

            def sample():
                ops.constrained_sample(logits, None, bank.next, bank.dist, DONE, st, rem, temp, seed, z[0], z[1], z[2],
                                       nout, outt)

            def update():
                ops.mirostat_update(logits, None, nout1, outt, temp, on, mu, tau, eta, m, lnz, mark)

            fns = {"restore": lambda: None, "mirostat_truncate": truncate, "constrained_sample": sample,
                   "mirostat_update": update}

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

            restore(); truncate(); sample(); update()  # noqa: E702 — warm-up (code objects); leaves mark and outt set
            kept = int((logits[0, :bank.next.shape[1]].float() > -math.inf).sum())
            moved = int((mu != mu0).sum())
            ts = {k: [] for k in fns}
            for _ in range(REPEATS):
                for k, fn in fns.items():  # interleaved: one repeat of each in turn
                    ts[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in ts.items()}
            base = med["restore"]
            tr_us, smp_us, up_us = (med[k] - base for k in ("mirostat_truncate", "constrained_sample",
                                                            "mirostat_update"))
            rec = dict(rows=rows, vocab=V, grammar=gname, legal_tokens=legal, tau=TAU, eta=ETA, mu=2 * TAU,
                       finite_logits_row0_after=kept, slots_whose_mu_moved=moved, launches=LAUNCHES, repeats=REPEATS,
                       restore_overhead_us=round(base, 2), mirostat_truncate_us=round(tr_us, 2),
                       constrained_sample_us=round(smp_us, 2), mirostat_update_us=round(up_us, 2),
                       truncate_over_sampler=round(tr_us / smp_us, 3), update_over_sampler=round(up_us / smp_us, 3),
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
