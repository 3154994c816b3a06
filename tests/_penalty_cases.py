"""Cases and oracle for ``ops.apply_penalties`` (csrc/kernels/penalties.hip; CPU: chronos.ops.reference), shared by
tests/test_penalties.py (CPU reference) and tests/test_penalties_gpu.py (HIP kernel).

The oracle is a plain per-row Python loop over the history window, stepping through llama.cpp's formula in fp32 (numpy
float32 scalars, one rounding per operation) and rounding to the logits dtype at the end.  Checks, per case:

* every logit outside the penalised set, and every row of a skipped or neutral slot, is BITWISE unchanged;
* penalised logits match the oracle to one unit in the last place of the logits dtype — relative 2^-8 for bf16, 1e-6
  for fp32 (room for an FMA contraction of ``c * fq + pr`` before the final rounding); non-finite values exactly;
* two launches on fresh copies of the same input give identical bits.
"""
import numpy as np
import torch

from chronos import ops

DONE = 0
CAP = ops.MAX_PENALTY_WINDOW
TOL = {"bf16": 2.0 ** -8, "f32": 1e-6}
DT = {"bf16": torch.bfloat16, "f32": torch.float32}


def oracle_row(row, hist, width, rp, fq, pr):
    """{token id: penalised fp32 value} of one logits row (fp32 list-like) under history ``hist`` (a list of ids)."""
    counts = {}
    for t in hist:
        if 0 <= t < width:
            counts[t] = counts.get(t, 0) + 1
    rp, fq, pr = np.float32(rp), np.float32(fq), np.float32(pr)
    out = {}
    with np.errstate(all="ignore"):
        for t, c in counts.items():
            x = np.float32(row[t])
            x = x * rp if x <= 0 else x / rp
            out[t] = np.float32(x - np.float32(np.float32(np.float32(c) * fq) + pr))
    return out


def history(case, slot):
    """The window the kernel must use for ``slot``: last L of prompt tail + generated, L clamped to W."""
    W, max_out = case["pen_tail"].shape[1], case["out_tokens"].shape[1]
    tl = int(case["pen_tlen"][slot])
    no = min(int(case["nout"][slot]), max_out)
    h = case["pen_tail"][slot, :tl].tolist() + case["out_tokens"][slot, :no].tolist()
    L = min(int(case["pen_last"][slot]), W)
    return h[-L:] if L > 0 else []


def live(case, slot):
    s = int(case["state"][slot])
    row = int(case["row_of_slot"][slot]) if case["row_of_slot"] is not None else slot
    rp, fq, pr = (float(v) for v in case["pen_par"][slot])
    neutral = rp == 1.0 and fq == 0.0 and pr == 0.0
    ok = s >= 0 and s != DONE and row >= 0 and not neutral and int(case["pen_last"][slot]) > 0
    return ok, row


def _logits(rows, width, dt, strided, gen):
    """[rows, width] logits of every kind (positive, negative, zero, -inf), as a view with a padded row stride when
    ``strided``."""
    full = torch.randn(rows, width + (24 if strided else 0), generator=gen) * 4.0
    full[:, ::7] = 0.0
    full[:, 3::11] = float("-inf")
    full[:, 5::13] = -0.0
    full = full.to(DT[dt])
    return full, (full[:, 8:8 + width] if strided else full)


def make(name, width, dt, slots, *, W=64, max_out=32, strided=False, perm=False, seed=0, fill=None):
    """A case dict (CPU tensors).  ``fill(case, gen)`` edits the per-slot state after the random default: every slot
    live, penalised with (1.3, 0.25, 0.5), L = W, a random prompt tail of random length and random output."""
    gen = torch.Generator().manual_seed(seed * 7919 + width + slots)
    rows = slots + (3 if perm else 0)
    full, view = _logits(rows, width, dt, strided, gen)
    hi = min(width, 50)  # a small id range, so tokens repeat inside a window
    c = dict(name=name, dt=dt, width=width, full=full, logits=view, row_of_slot=None,
             state=torch.randint(1, 9, (slots,), generator=gen, dtype=torch.int32),
             nout=torch.randint(0, max_out + 1, (slots,), generator=gen, dtype=torch.int32),
             out_tokens=torch.randint(0, hi, (slots, max_out), generator=gen, dtype=torch.int32),
             pen_par=torch.tensor([[1.3, 0.25, 0.5]] * slots, dtype=torch.float32),
             pen_last=torch.full((slots,), W, dtype=torch.int32),
             pen_tail=torch.randint(0, hi, (slots, W), generator=gen, dtype=torch.int32),
             pen_tlen=torch.randint(0, W + 1, (slots,), generator=gen, dtype=torch.int32))
    if perm:  # a permutation of the rows with -1 entries (slots not sampled in this launch)
        p = torch.randperm(rows, generator=gen)[:slots].to(torch.int32)
        p[1::3] = -1
        c["row_of_slot"] = p
    if fill:
        fill(c, gen)
    for s in range(slots):  # the tail past its valid length is padding the kernel must never read as history
        c["pen_tail"][s, int(c["pen_tlen"][s]):] = -1
    return c


def _window(L):
    def f(c, gen):
        c["pen_last"][:] = L
    return f


def _longer_than_history(c, gen):
    c["pen_tlen"][:] = 3
    c["nout"][:] = 2
    c["pen_last"][:] = 40


def _straddle(c, gen):  # the window takes the last outputs and reaches a few ids back into the prompt tail
    c["pen_tlen"][:] = c["pen_tail"].shape[1]
    c["nout"][:] = 5
    c["pen_last"][:] = 9


def _empty_tail(c, gen):
    c["pen_tlen"][:] = 0
    c["nout"].clamp_(min=1)


def _first_token(c, gen):
    c["nout"][:] = 0
    c["pen_tlen"].clamp_(min=1)


def _nothing_at_all(c, gen):
    c["nout"][:] = 0
    c["pen_tlen"][:] = 0


def _one_token_L_times(c, gen):
    W = c["pen_tail"].shape[1]
    c["pen_tail"][:] = 17
    c["out_tokens"][:] = 17
    c["pen_tlen"][:] = W
    c["pen_last"][:] = W


def _all_distinct(c, gen):
    W, mo = c["pen_tail"].shape[1], c["out_tokens"].shape[1]
    for s in range(c["state"].numel()):
        p = torch.randperm(c["width"], generator=gen)[:W + mo].to(torch.int32)
        c["pen_tail"][s], c["out_tokens"][s] = p[:W], p[W:]
    c["pen_tlen"][:] = W
    c["nout"][:] = mo


def _bad_ids(c, gen):  # padding ids and ids at or above the logits width, inside the valid history
    w = c["width"]
    c["pen_tlen"].clamp_(min=8)
    c["nout"].clamp_(min=6)
    for s in range(c["state"].numel()):
        c["pen_tail"][s, 0:4] = torch.tensor([-1, w, w + 5, 2 ** 31 - 1], dtype=torch.int32)
        c["out_tokens"][s, 0:4] = torch.tensor([-7, w, w - 1, 0], dtype=torch.int32)


def _rp_below_one(c, gen):
    c["pen_par"][:] = torch.tensor([0.7, 0.0, 0.0])


def _negative_fq_pr(c, gen):
    c["pen_par"][:] = torch.tensor([1.0, -0.375, -1.25])


def _each_alone(c, gen):  # one parameter off neutral per slot, non-dyadic values, and a fully neutral slot
    rows = [[1.1, 0.0, 0.0], [1.0, 0.1, 0.0], [1.0, 0.0, 0.3], [1.0, 0.0, 0.0]]
    for s in range(c["state"].numel()):
        c["pen_par"][s] = torch.tensor(rows[s % 4])


def _dead_slots(c, gen):  # DONE, empty, parked; a neutral slot and an L = 0 slot beside penalised ones
    n = c["state"].numel()
    kinds = [DONE, -1, -2, -9]
    for s in range(n):
        if s % 2:
            c["state"][s] = kinds[(s // 2) % 4]
    if n > 2:
        c["pen_par"][2] = torch.tensor([1.0, 0.0, 0.0])
    if n > 4:
        c["pen_last"][4] = 0


def cases():
    out = []
    k = 0
    for width in (1000, 1003):
        for dt in ("bf16", "f32"):
            k += 1
            st = dict(strided=(k % 2 == 0))
            out += [
                make("L1", width, dt, 1 + k, fill=_window(1), seed=k, **st),
                make("L64", width, dt, 2 + k, fill=_window(64), seed=k, **st),
                make("Lcap", width, dt, 3, W=CAP, max_out=48, fill=_window(CAP), seed=k, **st),
                make("L_above_W", width, dt, 2, W=40, fill=_window(CAP), seed=k, **st),
                make("L_longer_than_history", width, dt, 3, fill=_longer_than_history, seed=k, **st),
                make("straddle", width, dt, 4, fill=_straddle, seed=k, **st),
                make("empty_tail", width, dt, 5, fill=_empty_tail, seed=k, **st),
                make("first_token", width, dt, 3, fill=_first_token, seed=k, **st),
                make("no_history", width, dt, 2, fill=_nothing_at_all, seed=k, **st),
                make("count_L", width, dt, 2, fill=_one_token_L_times, seed=k, **st),
                make("count_cap", width, dt, 1, W=CAP, max_out=8, fill=_one_token_L_times, seed=k, **st),
                make("all_distinct", width, dt, 3, fill=_all_distinct, seed=k, **st),
                make("bad_ids", width, dt, 4, fill=_bad_ids, seed=k, **st),
                make("rp_below_one", width, dt, 3, fill=_rp_below_one, seed=k, **st),
                make("negative_fq_pr", width, dt, 3, fill=_negative_fq_pr, seed=k, **st),
                make("each_alone", width, dt, 8, fill=_each_alone, seed=k, **st),
                make("perm", width, dt, 7, perm=True, seed=k, **st),
                make("dead_slots", width, dt, 9, fill=_dead_slots, seed=k, **st),
                make("dead_slots_perm", width, dt, 9, perm=True, fill=_dead_slots, strided=not st["strided"], seed=k),
            ]
    out.append(make("llama3_vocab", 128256, "bf16", 2, W=CAP, max_out=16, seed=99,
                    fill=lambda c, gen: c["pen_tail"].copy_(torch.randint(0, 128256, c["pen_tail"].shape, generator=gen,
                                                                          dtype=torch.int32))))
    return out


def case_id(c):
    return f"{c['name']}-{c['width']}-{c['dt']}-{c['state'].numel()}s" + ("-strided" if c["full"] is not c["logits"] else "")


def launch(case, dev):
    """Run the op on a fresh copy of the case's tensors on ``dev``; returns the whole (padded) logits buffer on the
    host, so writes outside the view would show too."""
    mv = lambda t: None if t is None else t.clone().to(dev)  # noqa: E731
    full = mv(case["full"])
    off = case["logits"].storage_offset() - case["full"].storage_offset()
    view = full.as_strided(case["logits"].shape, case["logits"].stride(), full.storage_offset() + off)
    ops.apply_penalties(view, mv(case["row_of_slot"]), DONE, mv(case["state"]), mv(case["nout"]),
                        mv(case["out_tokens"]), mv(case["pen_par"]), mv(case["pen_last"]), mv(case["pen_tail"]),
                        mv(case["pen_tlen"]))
    if dev != "cpu":
        torch.cuda.synchronize()
    return full.cpu()


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check(case, dev):
    got_full = launch(case, dev)
    again = launch(case, dev)
    assert torch.equal(bits(got_full), bits(again)), "two launches on the same input differ"
    off = case["logits"].storage_offset() - case["full"].storage_offset()
    got = got_full.as_strided(case["logits"].shape, case["logits"].stride(), off)
    before = case["logits"]
    touched = torch.zeros(case["full"].shape, dtype=torch.bool)
    tview = touched.as_strided(before.shape, before.stride(), off)
    tol, npen = TOL[case["dt"]], 0
    for slot in range(case["state"].numel()):
        ok, row = live(case, slot)
        if not ok:
            continue
        want = oracle_row(before[row].float().tolist(), history(case, slot), case["width"],
                          *(float(v) for v in case["pen_par"][slot]))
        for t, w in want.items():
            tview[row, t] = True
            npen += 1
            w = float(torch.tensor(float(w)).to(before.dtype))  # the final rounding to the row's dtype
            g = float(got[row, t])
            if not np.isfinite(w) or w == 0.0:
                assert g == w or (np.isnan(w) and np.isnan(g)), (case_id(case), slot, t, g, w)
            else:
                assert abs(g - w) <= tol * abs(w), (case_id(case), slot, t, g, w)
    same = bits(got_full) == bits(case["full"])
    assert bool(same[~touched].all()), "a logit outside the penalised set changed"
    return npen
