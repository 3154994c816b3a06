"""Shared cases for tests/test_sampler_replay.py (CPU) and tests/test_sampler_replay_gpu.py (the HIP kernel): the
sampled half of csrc/kernels/sampler.hip, checked token by token.

The kernel's noise is a counter hash of (seed, nout, slot, token), a pure integer function, so the host replays it bit
for bit (chronos.ops.reference.sampler_uniform) and scores every token in fp64: ``x / T - log(-log(u))``.  The device
evaluates the same expression in fp32 with fast logarithms, so its token must be the fp64 argmax or lie within G of it
(``judge``).  A wrong stream, a wrong temperature or a wrong token index moves scores by O(0.1 - 1) and is rejected in
most rows (tests/test_sampler_replay.py measures that on mutated samplers); fp32 evaluation moves them by far less.

G is measured, not guessed: tests/test_sampler_replay_gpu.py records the largest fp64 gap among the rows where the
device's token is not the fp64 argmax (profiles/sampler/replay_gap.json), and G is 4x that, at least 2^-16 and at most
2^-7.  A disagreement above 2^-7 is a failure whatever was measured.
"""
import json
import math
import os

import numpy as np
import torch

from chronos import ops
from chronos.ops import reference as ref

from _truncate_cases import DONE, NEG, REMAINING, ST_GEN, ST_NEAR, Slots, build_dfa, ladder_row, legal_mask

M32 = 0xFFFFFFFF
G_FLOOR, G_CAP = 2.0 ** -16, 2.0 ** -7
GAP_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler",
                        "replay_gap.json")


def g_from_gap(max_gap: float) -> float:
    return min(G_CAP, max(G_FLOOR, 4.0 * max_gap))


# g_from_gap(largest gap in profiles/sampler/replay_gap.json); tests/test_sampler_replay.py checks that.  The first
# run on an MI355X, at G = 2^-7, found the device on the fp64 argmax in every one of its 2 740 sampled rows (largest
# gap 0), so G is the floor.
G = 2.0 ** -16

SEEDS = (0, 1, -1, -2 ** 31, 2 ** 31 - 1, 12345, -77)
NOUTS = (0, 1, 63, 2 ** 20, 2)
TEMPS = (0.25, 0.7, 1.0, 1.3, 4.0)
MAX_OUT = 64

# (seed, nout, slot, token) at which the parent's uniform was 1.0f (hash >> 8 == 2^24 - 1): the token won whatever
# its logit
OLD_HITS = {128256: [(62, 0, 0, 77271), (99, 0, 0, 57213), (111, 0, 0, 40565)],
            1003: [(3789, 0, 0, 718), (26405, 0, 0, 128), (37245, 0, 0, 398)]}


# ---- the hash a second time: plain Python ints, written from the kernel text ---------------------------------------
def mix32_int(x: int) -> int:
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def hash_int(seed: int, nout: int, slot: int, v: int) -> int:
    key = mix32_int((((seed & M32) * 0x9E3779B9) & M32) ^ (((nout & M32) * 0x85EBCA6B) & M32) ^ (slot & M32))
    return mix32_int(key ^ (((v & M32) * 0xC2B2AE35) & M32))


def hash_tuples():
    return [(s, n, b, v) for s in SEEDS for n in NOUTS[:4] for b in (0, 1, 255, 4095) for v in (0, 1, 1002, 128255)]


# ---- the uniform as a function of the shifted hash, numpy fp32 ------------------------------------------------------
NEW_SHIFT, OLD_SHIFT = 9, 8


def uniform_np(h: np.ndarray) -> np.ndarray:
    """The kernel's u of h = hash >> 9 (h < 2^23)."""
    return (h.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def uniform_old_np(h: np.ndarray) -> np.ndarray:
    """Frozen copy of the parent's formula, u of h = hash >> 8 (h < 2^24): kept as a mutation that the soundness
    check must reject (h + 0.5 is not representable from 2^23 on and rounds to even; at 2^24 - 1 it gives u = 1)."""
    return (h.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def uniform_is_sound(u: np.ndarray) -> bool:
    """0 < u < 1, strictly increasing in h, and a finite Gumbel value at both ends (fp32)."""
    with np.errstate(divide="ignore"):
        gum = -np.log(-np.log(u[[0, -1]]))
    return bool(u.dtype == np.float32 and (u > 0).all() and (u < 1).all() and (np.diff(u) > 0).all()
                and np.isfinite(gum).all())


# ---- replay and acceptance ------------------------------------------------------------------------------------------
def gumbel_scores(x: torch.Tensor, keep: torch.Tensor, T: float, u: torch.Tensor) -> torch.Tensor:
    s = x.float().double() / T - torch.log(-torch.log(u.double()))
    return s.masked_fill(~keep, NEG)


def replay(logits_row, legal, T, seed, nout, slot) -> torch.Tensor:
    """fp64 scores x / T - log(-log(u)) of one row: x the fp32 value of the logit, u the kernel's uniform; tokens
    outside ``legal`` (illegal or filtered out) get -inf."""
    return gumbel_scores(logits_row, legal, T, ref.sampler_uniform(seed, nout, slot, logits_row.numel()))


def judge(s64: torch.Tensor, t: int, g: float):
    """(accepted, gap): the token is a legal survivor and scores within g of the fp64 maximum."""
    if not (0 <= t < s64.numel()) or float(s64[t]) == NEG:
        return False, math.inf
    gap = float(s64.max() - s64[t])
    return gap <= g, gap


def top_two_gap(s64: torch.Tensor) -> float:
    top = torch.topk(s64, 2).values
    return float(top[0] - top[1])


def survivors(x: torch.Tensor, legal: torch.Tensor, tk: int, tp: float) -> torch.Tensor:
    if tk <= 0 and tp >= 1.0:
        return legal
    return legal & (ref.ord_key(x.float()) >= ref.topkp_threshold(x.float(), legal, tk, tp))


def ladder_topp(x: torch.Tensor, legal: torch.Tensor, j: int) -> float:
    """A top_p whose nucleus ends with the j-th key class (descending), halfway through that class's mass, with the
    margin asserted: the kernel's fp32 mass sums (LDS atomics, order not fixed) cannot move the threshold."""
    keys = ref.ord_key(x.float())[legal]
    p = torch.softmax(x.double()[legal], 0)
    uk, inv = torch.unique(keys, return_inverse=True)
    mass = torch.zeros(uk.numel(), dtype=torch.float64).index_add_(0, inv, p).flip(0)  # descending keys
    cum = torch.cumsum(mass, 0)
    upto, below = float(cum[j]), float(cum[j - 1]) if j else 0.0
    tp = float(torch.tensor((below + upto) / 2, dtype=torch.float32))
    assert tp - below >= 1e-3 and upto - tp >= 1e-3, ("mass margin", tp - below, upto - tp)
    assert ref.topkp_threshold(x.float(), legal, 0, tp) == int(uk.flip(0)[j])
    return tp


# ---- slot builders --------------------------------------------------------------------------------------------------
MUTABLE = ("state", "rem", "ids", "pos", "ctx", "nout", "ring")


class Case(Slots):
    """``n`` slots in the mix of _truncate_cases.Slots (DONE, parked, empty, unsampled, greedy, sampled; poison in the
    logits padding; ``rows`` "perm" or None), one logits row of its own per slot, temperatures, seeds and ``nout``
    cycled over the slots (periods 5, 7, 5 against the kinds' 8).  ``filt``: "none", "topk" (1, 4, 40 cycled), "topp"
    (ladder rows, ``ladder_topp``), "both" (top_k 4 over the ladder rows).  ``done`` of the legal tokens close the
    row (next state DONE), in both live states; with ``jump`` a row that enters ST_NEAR is parked."""

    def __init__(self, vocab, dt, n=256, temps=TEMPS, filt="none", rows="perm", case_seed=0, all_live=False,
                 jump=False, done=0.05, remaining=REMAINING, nouts=NOUTS):
        g = torch.Generator().manual_seed(1000 + case_seed)
        nxt, dist = build_dfa(vocab, g)
        closing = (torch.rand(vocab, generator=g) < done) & (nxt[ST_GEN] == ST_NEAR)
        nxt[ST_GEN][closing] = DONE
        nxt[ST_NEAR] = nxt[ST_GEN]
        legal = legal_mask(nxt, dist, ST_GEN, remaining)
        if filt in ("topp", "both"):
            base = [ladder_row(vocab, legal, g) for _ in range(16)]
            x = [base[s % 16] for s in range(n)]
        else:
            xr = torch.randn(n, vocab, generator=g) * 2.0
            xr[:, (~legal).nonzero().flatten()[0]] = 60.0  # an illegal token holds the largest logit of every row
            x = list(xr)
        super().__init__(n, vocab, dt, "cpu", nxt, dist, ST_GEN, x, minp=(0.0,), typ=(1.0,), rows=rows,
                         remaining=remaining)
        if all_live:
            self.kinds = ["live"] * n
            self.state_c = torch.full((n,), ST_GEN, dtype=torch.int32)
            self.row_c = torch.tensor(self.perm, dtype=torch.int32)
        if rows is None:  # without row_of_slot every slot reads the row of its own index
            self.kinds = ["live" if k == "norow" else k for k in self.kinds]
        self.filt, self.dt = filt, dt
        self.temp_c = torch.tensor([0.0 if k == "greedy" else temps[s % len(temps)]
                                    for s, k in enumerate(self.kinds)])
        self.seed_c = torch.tensor([SEEDS[s % len(SEEDS)] for s in range(n)], dtype=torch.int32)
        self.nout_c = torch.tensor([nouts[s % len(nouts)] for s in range(n)], dtype=torch.int32)
        self.topk_c = torch.zeros(n, dtype=torch.int32)
        self.topp_c = torch.ones(n)
        if filt == "topk":
            self.topk_c = torch.tensor([(1, 4, 40)[s % 3] for s in range(n)], dtype=torch.int32)
        if filt in ("topp", "both"):
            tps = [ladder_topp(base[r], legal, (0, 1, 3, 8)[r % 4]) for r in range(16)]
            self.topp_c = torch.tensor([tps[s % 16] for s in range(n)])
        if filt == "both":
            self.topk_c = torch.full((n,), 4, dtype=torch.int32)
        self.jump_c = torch.tensor([0, 0, 3, 0, 0], dtype=torch.int16) if jump else None
        self.ids_c = torch.zeros(n, dtype=torch.int32)
        self.pos_c = torch.arange(n, dtype=torch.int32)
        self.ctx_c = self.pos_c + 1
        self.ring_c = torch.full((n, MAX_OUT), -1, dtype=torch.int32)

    # -- host side --
    def start(self):
        """The mutable per-slot state, as a dict of fresh host tensors."""
        return {k: getattr(self, k + "_c").clone() for k in MUTABLE}

    def row(self, slot, buf=None):
        """fp32 values of the slot's logits row (of ``buf``, default the case's own)."""
        r = self.perm[slot] if self.rows == "perm" else slot
        return (self.buf_c if buf is None else buf)[r, :self.vocab].float()

    def active(self, st):
        s = st["state"]
        live = (s > 0) & (s != DONE)
        return [i for i in range(self.n) if bool(live[i]) and (self.rows != "perm" or int(self.row_c[i]) >= 0)]

    def sampled(self, st=None):
        st = st or self.start()
        return [i for i in self.active(st) if float(self.temp_c[i]) > 0]

    def scores(self, slot, st=None, buf=None):
        """fp64 replay of one sampled slot at the state ``st`` (default: the case's start)."""
        st = st or self.start()
        x = self.row(slot, buf)
        legal = legal_mask(self.nxt_c, self.dist_c, int(st["state"][slot]), int(st["rem"][slot]))
        keep = survivors(x, legal, int(self.topk_c[slot]), float(self.topp_c[slot]))
        return replay(x, keep, float(self.temp_c[slot]), int(self.seed_c[slot]), int(st["nout"][slot]), slot)

    def advance(self, st, slot, t):
        """What the kernel writes for ``slot`` when it picks token ``t``, applied to ``st`` in place."""
        ns = int(self.nxt_c[int(st["state"][slot]), t])
        k = int(st["nout"][slot])
        if k < MAX_OUT:
            st["ring"][slot, k] = t
        st["nout"][slot] = k + 1
        st["rem"][slot] -= 1
        park = self.jump_c is not None and ns != DONE and 0 < int(self.jump_c[ns]) <= int(st["rem"][slot])
        st["state"][slot] = -2 - ns if park else ns
        if ns != DONE:
            st["ids"][slot] = t
            st["pos"][slot] += 1
            st["ctx"][slot] += 1

    def check_step(self, before, after, g, buf=None, gaps=None):
        """One launch judged slot by slot.  Inactive slots: nothing moved.  Greedy slots: the smallest id among the
        largest legal logits.  Sampled slots: ``judge`` against the fp64 replay; a token that is not the replay's
        argmax is recorded in ``gaps`` as (slot, gap).  Every active slot: all of its state advanced as ``advance``
        does for the device's token."""
        want = {k: v.clone() for k, v in before.items()}
        act = set(self.active(before))
        bad = []
        for slot in act:
            k = int(before["nout"][slot])
            assert int(after["nout"][slot]) == k + 1, ("nout", slot)
            # the device's token: in the ring, or past its end in ids (a row that closed there shows no token)
            t = int(after["ring"][slot, k]) if k < MAX_OUT else (
                int(after["ids"][slot]) if int(after["state"][slot]) != DONE else None)
            if float(self.temp_c[slot]) > 0:
                s64 = self.scores(slot, before, buf)
                if t is None:  # closed past the ring: the replay's near-maximal tokens must include a closing one
                    near = (s64 >= s64.max() - g).nonzero().flatten()
                    t = next((int(v) for v in near if int(self.nxt_c[int(before["state"][slot]), v]) == DONE), -1)
                ok, gap = judge(s64, t, g)
                if not ok:
                    bad.append((slot, t, int(s64.argmax()), gap))
                    continue
                if gap > 0 and gaps is not None:
                    gaps.append((slot, gap))
            else:
                x = self.row(slot, buf)
                legal = legal_mask(self.nxt_c, self.dist_c, int(before["state"][slot]), int(before["rem"][slot]))
                xl = x.masked_fill(~legal, NEG)
                first = int((xl == xl.max()).nonzero()[0])
                t = first if t is None else t
                assert t == first, ("greedy", slot, t, first)
            self.advance(want, slot, t)
        assert not bad, f"sampled rows rejected at G = {g}: (slot, token, replay argmax, gap) {bad[:8]} of {len(bad)}"
        for k in MUTABLE:
            assert torch.equal(after[k], want[k]), (k, (after[k] != want[k]).nonzero().flatten().tolist()[:8])

    # -- either backend --
    def launch(self, dev, st, buf=None):
        """ops.constrained_sample on ``dev`` over the state ``st`` (a dict on ``dev``, advanced in place)."""
        d = lambda t: None if t is None else t.to(dev)  # noqa: E731
        buf = d(self.buf_c.clone()) if buf is None else buf
        logits = buf[:, :self.vocab] if self.rows == "perm" else buf[:self.n, :self.vocab]
        ops.constrained_sample(logits, d(self.row_c) if self.rows == "perm" else None, d(self.nxt_c), d(self.dist_c),
                               DONE, st["state"], st["rem"], d(self.temp_c), d(self.seed_c), st["ids"], st["pos"],
                               st["ctx"], st["nout"], st["ring"], d(self.topk_c), d(self.topp_c), d(self.jump_c))

    def run(self, dev):
        """One launch from the start state; (before, after) on the host."""
        before = self.start()
        st = {k: v.clone().to(dev) for k, v in before.items()}
        self.launch(dev, st)
        return before, {k: v.cpu() for k, v in st.items()}


# The one-step cases of the GPU test (tests/test_sampler_replay.py checks their near-tie share on the CPU).  V = 1003
# takes the kernel's non-vector instantiation, V = 1024 the vector one (sampled rows on its general loop).
GPU_CASES = [dict(vocab=v, dt=dt, filt=f, rows=r, jump=(r is None), case_seed=i)
             for i, (v, dt, f, r) in enumerate([
                 (1003, "bf16", "none", "perm"), (1003, "f32", "none", None), (1024, "bf16", "none", None),
                 (1024, "f32", "none", "perm"), (1003, "bf16", "topk", "perm"), (1024, "f32", "topk", None),
                 (1003, "f32", "topp", "perm"), (1024, "bf16", "topp", None), (1003, "bf16", "both", None),
                 (1024, "f32", "both", "perm")])]


def case_id(kw):
    return f"v{kw['vocab']}-{kw['dt']}-{kw['filt']}-{'perm' if kw['rows'] else 'norows'}"


def multi_step_case(vocab, dt):
    """64 slots for forty launches with the state carried: ``nout`` starts at 0 (the ring holds every token), budget
    45, 1 % of the legal tokens close a row."""
    return Case(vocab, dt, n=64, filt="none", rows="perm", case_seed=77, done=0.01, remaining=45, nouts=(0,))


def step_logits(c, step):
    """The logits buffer of launch ``step`` of the multi-step test (fresh values in the rows, poison kept)."""
    g = torch.Generator().manual_seed(5000 + step)
    buf = c.buf_c.clone()
    buf[:, :c.vocab] = (torch.randn(buf.shape[0], c.vocab, generator=g) * 2.0).to(buf.dtype)
    return buf


def forced_case(vocab, hit):
    """One slot at (seed, 0, 0) with the hit token legal and 30 below every other logit, temperature 1: the parent's
    u = 1 made its score +inf; with u < 1 its noise is at most -log(-log(1 - 2^-24)) = 16.6 and the other tokens'
    at least -log(-log(2^-24)) = -2.8, so it loses to every legal token."""
    seed, nout, slot, tok = hit
    assert nout == 0 and slot == 0
    c = Case(vocab, "bf16", n=1, temps=(1.0,), rows=None, case_seed=tok, done=0.0, nouts=(0,))
    c.seed_c[0] = seed
    c.nxt_c[ST_GEN, tok] = ST_NEAR
    c.buf_c[0, tok] = float(c.buf_c[0, :vocab].float().min()) - 30.0
    assert bool(legal_mask(c.nxt_c, c.dist_c, ST_GEN, REMAINING)[tok])
    return c, tok


# ---- mutated samplers (the yardstick must notice them) --------------------------------------------------------------
def mutant_token(c, slot, how):
    """The token a subtly wrong sampler would draw for a sampled slot of ``c`` at its start state."""
    x = c.row(slot)
    keep = survivors(x, c.legal, int(c.topk_c[slot]), float(c.topp_c[slot]))
    T, seed, nout, V = float(c.temp_c[slot]), int(c.seed_c[slot]), int(c.nout_c[slot]), c.vocab
    if how == "greedy":
        return int(x.masked_fill(~keep, NEG).argmax())
    if how == "temperature":
        T *= 1.25
    u = {"nout": lambda: ref.sampler_uniform(seed, 0, slot, V),
         "slot": lambda: ref.sampler_uniform(seed, nout, 0, V),
         "token": lambda: ref.sampler_uniform(seed, nout, slot, V + 1)[1:]}.get(
             how, lambda: ref.sampler_uniform(seed, nout, slot, V))()
    return int(gumbel_scores(x, keep, T, u).argmax())


MUTANTS = ("nout", "slot", "token", "temperature", "greedy")


def load_gaps():
    with open(GAP_FILE) as fh:
        return json.load(fh)
