"""Cost of per-token logprobs (csrc/kernels/logprobs.hip) next to the sampler they bracket, on the Llama-3 vocabulary.

One process, the three kernels interleaved: token_logprobs (before the sampler), constrained_sample (greedy),
token_logprobs_commit (after it), at 1 row (single stream) and 1024 rows (the wave), top 5 and top 20, for three
grammars: the verdict schema's start state (few legal tokens), the free grammar, and a synthetic automaton with every
token id legal (the pre-kernel's worst case: all 128 256 logits enter the logsumexp and the select).  Every launch
starts from the same slot state (a few tiny device copies restore it; the same copies precede every timed launch and
their own cost is measured and subtracted), device events around 50 launches, median of 7 repeats after a warm-up.

    python scripts/bench_logprobs.py [--out profiles/logprobs/kernel_cost.jsonl]
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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_logprobs.py measures GPU kernels: no GPU found")
    from chronos import ops
    from chronos.brain.constrain import DONE, GrammarBank
    from chronos.brain.tokenizer import load_tokenizer
    from chronos.sensor.prompt import VERDICT_SCHEMA

    ops.load()
    tok = load_tokenizer(None)
    bank = GrammarBank(tok.token_bytes_list(), tok.stop_ids, V, 1024, "cuda")
    # (next table, dist table, start state): the verdict schema, the free grammar over the tokenizer's real tokens, and
    # a synthetic automaton in which all 128 256 ids are legal
    all_next = torch.ones(2, V, dtype=torch.int16, device="cuda")
    all_dist = torch.tensor([0, 1], dtype=torch.int16, device="cuda")
    grammars = {"verdict": (bank.next, bank.dist, bank.get(VERDICT_SCHEMA).start),
                "free": (bank.next, bank.dist, bank.get(None).start), "all_legal": (all_next, all_dist, 1)}
    i32 = dict(dtype=torch.int32, device="cuda")
    recs = []
    for rows in a.rows:
        logits = torch.randn(rows, V, device="cuda").to(torch.bfloat16)
        for grammar, (nxt, dst, start) in grammars.items():
            for K in (5, 20):
                st0, rem0, nout0 = torch.full((rows,), start, **i32), torch.full((rows,), 60, **i32), \
                    torch.zeros(rows, **i32)
                st, rem, nout = st0.clone(), rem0.clone(), nout0.clone()
                z = [torch.zeros(rows, **i32) for _ in range(3)]
                outt = torch.zeros(rows, MAX_OUT, **i32)
                want = torch.full((rows,), K, **i32)
                mark, lse = torch.full((rows,), -1, **i32), torch.zeros(rows, device="cuda")
                tid, tval = torch.zeros(rows, K, **i32), torch.zeros(rows, K, device="cuda")
                ring = torch.zeros(rows, MAX_OUT, 1 + K, device="cuda")
                ring_ids = torch.zeros(rows, MAX_OUT, K, **i32)
                nout1 = nout0 + 1  # what the sampler leaves: the commit kernel writes entry 0 of every row

                def restore():
                    st.copy_(st0)
                    rem.copy_(rem0)
                    nout.copy_(nout0)

                def pre():
                    ops.token_logprobs(logits, None, nxt, dst, DONE, st, rem, nout, want, mark, lse, tid,
                                       tval)

                def sample():
                    ops.constrained_sample(logits, None, nxt, dst, DONE, st, rem, None, None, z[0], z[1],
                                           z[2], nout, outt)

                def commit():
                    nout.copy_(nout1)
                    ops.token_logprobs_commit(logits, None, nout, outt, want, mark, lse, tid, tval, ring, ring_ids)

                fns = {"restore": lambda: None, "token_logprobs": pre, "constrained_sample": sample,
                       "token_logprobs_commit": commit}

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

                restore(); pre(); sample(); commit()  # noqa: E702 — warm-up (code objects), and a mark for the commit
                restore(); pre()  # noqa: E702
                ts = {k: [] for k in fns}
                for _ in range(REPEATS):
                    for k, fn in fns.items():  # interleaved: one repeat of each in turn
                        ts[k].append(timed(fn))
                med = {k: statistics.median(v) for k, v in ts.items()}
                base = med["restore"]
                # the commit's timed body carries one more tiny copy (nout) than the others: ~ a third of the restore
                rec = dict(rows=rows, vocab=V, grammar=grammar, top=K, launches=LAUNCHES, repeats=REPEATS,
                           legal_tokens=int((nxt[start].long() >= 0).sum()),
                           restore_overhead_us=round(base, 2),
                           token_logprobs_us=round(med["token_logprobs"] - base, 2),
                           constrained_sample_us=round(med["constrained_sample"] - base, 2),
                           token_logprobs_commit_us=round(med["token_logprobs_commit"] - base * 4 / 3, 2),
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
