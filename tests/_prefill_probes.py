"""Exact per-key probes for prefill attention (csrc/kernels/attention_prefill.hip: attn_prefill_kernel,
attn_prefill2_kernel, attn_prefill8_kernel; csrc/kernels/attention.hip: paged_attn_kernel<2>), shared by
tests/test_prefill_probes.py (CPU: builders, closed forms, coverage and mutation checks against chronos.ops.reference)
and tests/test_prefill_probes_gpu.py (the HIP kernels).  The decode probes (tests/_decode_probes.py) explain why random
K / V under ``atol 2e-2`` (or, for the fp8-MFMA kernels, a 5 % norm bound) cannot see one dropped, doubled, stale or
mis-paired key; the pieces that carry over (``code_rows``, ``u_counts``, ``_store``, ``_load``, the poison value and the
bounds) are imported from there.  D = 128, page size 16 or 32, block ids randomly permuted; every stored value is exact
in bf16 AND in e4m3 at the power-of-two cache scales k_scale = 4, v_scale = 0.5 (passed separately, and different).

U (uniform) — which keys are attended.  K = 0 at every valid position, V[h][t, d] = 1 iff d == (t + 5 h) % 128, q random
    from Q_VALUES with one sign per dim.  Expected output = u_counts(L, h) / L with L = ctx - (n - 1 - i) the causal
    length of token i of an n-token chunk: any key read past the causal diagonal, past kv_end or dropped at a stage edge
    changes an integer count.
C (comb) — which V goes with which K, for any number of query rows per kv head.  H = the 128 x 128 Sylvester Hadamard
    matrix (entries +-1, rows orthogonal, column 0 all +1).  The key at position t of kv head h is K = b H[cls(t, h)],
    cls(t, h) = (t + 3 h) % 128, and V[h][t] = code_rows(t + 5 h).  Query row (token i, head hd) is q = a H[c] for a
    class c the builder picks, a b = 4 (a = 1, b = 4): a key of class c scores a b 128 / sqrt(128) = 45.3 nat = 65.3
    log2 units, every other key scores exactly 0 (``margin_log2`` asserts both in fp64 on the dequantised tensors).
    Expected output = the mean of the code rows of the visible keys (t < L) of class c: positions t0, t0 + 128, ... —
    1 to 9 rows at the probes' contexts.  The heads of a token sweep the distance s from the diagonal, c =
    cls(L - 1 - s): s in SWEEP, s = -1 where L > 128 (the class of the first masked key, which must NOT appear in the
    mean), then the absolute positions of ``_extras`` (first key, page / step edges, both sides of the cached-prefix
    boundary, 1023 / 1024 / 1025, the kv-split edges); the sweep is rotated per token so every s meets every row
    parity and wave.
    The fp8-MFMA kernels quantise q per row to e4m3: all 128 entries of a comb q share one magnitude, so whatever
    the row's scale is they map to one e4m3 magnitude again — q stays a multiple of H[c], the zero scores stay exactly
    zero (orthogonality needs only equal magnitudes) and the needle score moves by at most e4m3's 2^-4 relative
    rounding of that one magnitude, 65.3 -> above 61 log2 units.

Poison (both probes): every cache block outside all block tables (the table padding points at one), every slot at or
past ctx in a sequence's last page, and with them every page past kv_end that a clamped or over-long stage could reach
through the padding, hold K = 128 b e_0 (column 0 of H is +1 and the U probe's q[.., 0] > 0: every row scores it as
high as a needle, or higher) and V = 64.0, finite.  A masked read contributes exactly 0, an unmasked one swamps the
output.

Bounds (derived, not measured).  Scores are exactly 0 or one shared value per row, so p = 2^0 for every key that
counts (exact in bf16 and in e4m3), the row sum l is an exact small integer (the fp8 kernels' ones-MFMA row sum
included) and O is an exact integer (U) / an exact sum of at most 9 half-integer code rows plus a leak below
L 2^-61 7.5 (C) in fp32.  What rounds: the 1 / l multiply (and the folded v_scale, a power of two) — a few 2^-24;
under a kv split the combine's exp2 / log2 — a few 2^-22; and the round-to-nearest bf16 store of the output, at most
2^-9 relative.  All of it is strictly inside the decode probes' bounds, which hold here unchanged:
    U: |out - e| <= 2^-7 e   + 1e-6   (L <= 2200 -> count <= 18: one wrong key moves a hit dim by >= 1/18 relative,
                                       seven times the bound; count = 0 dims must be 0 within 1e-6)
    C: |out - e| <= 2^-7 |e| + 2^-7   (|e| <= 7.5: at most 0.066.  One lost, extra or exchanged member among n <= 9
                                       (L <= 1133) moves the mean by |v - e'| / (n +- 1) or |v - v'| / n with v, v'
                                       code rows and e' a mean of others: two code rows differ by >= 1 in most dims,
                                       >= 1 / 9 = 0.11; the CPU mutation tests assert, by enumeration, a factor >= 2
                                       over the bound for EVERY affected row)
"""
from __future__ import annotations

import dataclasses
import functools
import math

import torch

from chronos.ops import reference as ref

from _decode_probes import (D, KV_SCALE, LOG2E, N_ABS, N_REL, POISON_V, Q_VALUES, U_ABS, U_REL, _load, _store,
                            code_rows, split_edges, u_counts)

A_Q, B_K = 1.0, 4.0  # comb amplitudes: q = A_Q H[c], K = B_K H[cls]
K_SCALE, V_SCALE = 4.0, KV_SCALE  # fp8 cache scales: K entries 4 -> 1, K poison 512 -> 128, V <= 7.5 -> 15, 64 -> 128
POISON_K0 = 128.0 * B_K  # dim 0 of a poison key
SWEEP = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127)
MAX_CTX = 2200
NSPLITS = (3, 8)  # the kv splits the nqt = 2 tests launch


@functools.lru_cache(maxsize=None)
def hadamard() -> torch.Tensor:
    i = torch.arange(D)
    x = i[:, None] & i[None, :]
    par = torch.zeros_like(x)
    for b in range(7):
        par ^= (x >> b) & 1
    return 1.0 - 2.0 * par.float()


def cls(t, h):
    return (t + 3 * h) % D


@dataclasses.dataclass
class Probe:
    kind: str  # "U" | "C"
    hq: int
    hkv: int
    bs: int
    fp8: bool
    q: torch.Tensor  # [T, hq, 128] bf16
    k: torch.Tensor  # [nb, hkv, bs, 128] bf16 / e4m3 bytes
    v: torch.Tensor  # [nb, hkv, 128, bs]
    bt: torch.Tensor  # [B, W] int32, padded with the id of a poison block
    qs: torch.Tensor  # [B + 1] int32
    ctx: torch.Tensor  # [B] int32
    q_lens: list
    prefix: list
    lens: list  # causal length L of every token
    expect: torch.Tensor  # [T, hq, 128] f32 closed form
    t0: torch.Tensor | None  # C: [T, hq] first position of the row's class (its members are t0 + 128 j < L)
    sdist: torch.Tensor | None  # C: [T, hq] the distance from the diagonal the builder aimed at (L - 1 - s is a member)
    pad: int

    @property
    def B(self) -> int:
        return len(self.q_lens)

    @property
    def scales(self):
        return (K_SCALE, V_SCALE) if self.fp8 else (1.0, 1.0)

    @property
    def seq_of(self) -> list:
        return [b for b, n in enumerate(self.q_lens) for _ in range(n)]


def _extras(L, ctx0, kv_end, splits):
    """Absolute positions the sweep also aims at: the first key, a page / 32 / 64-key step edge, both sides of the
    boundary between the cached prefix and the chunk, the 1024-token window, the kv-split edges of the row's tile."""
    out = [0, 15, 16, 31, 32, 63, 64, ctx0 - 1, ctx0, 1023, 1024, 1025]
    if splits:
        out += split_edges(kv_end, NSPLITS)[:6]
    return [p for p in out if 0 <= p < L]


def build(kind: str, q_lens, prefix, hq: int, hkv: int, *, bs: int = 16, fp8: bool = False, seed: int = 0,
          width: int | None = None, splits: bool = False) -> Probe:
    """One launch's probe on the CPU: chunks of q_lens tokens on cached prefixes of ``prefix`` tokens.  ``splits``: the
    sweep also aims at the kv-split edges of the row's 32-row tile (paged_attn_kernel<2>: chunk = ceil(kv_end / nsplit)
    rounded up to 32, kv_end the tile's last causal length)."""
    assert kind in ("U", "C") and hq % hkv == 0 and bs in (16, 32)
    g = torch.Generator().manual_seed(seed)
    B, G = len(q_lens), hq // hkv
    q_lens, prefix = list(q_lens), list(prefix)
    ctx = [p + n for p, n in zip(prefix, q_lens)]
    assert min(q_lens) >= 1 and max(ctx) <= MAX_CTX
    T = sum(q_lens)
    qs = [0]
    for n in q_lens:
        qs.append(qs[-1] + n)
    lens = [c - (n - 1 - i) for c, n in zip(ctx, q_lens) for i in range(n)]

    # ---- block tables: randomly permuted ids, the padding -> a poison block
    nbs = [(c + bs - 1) // bs for c in ctx]
    nb = sum(nbs) + 3
    perm = torch.randperm(nb, generator=g).tolist()
    pad = perm[-1]
    W = width if width is not None else max(nbs)
    assert W >= max(nbs)
    bt = torch.full((B, W), pad, dtype=torch.int32)
    nxt = 0
    for b, n in enumerate(nbs):
        bt[b, :n] = torch.tensor(perm[nxt:nxt + n], dtype=torch.int32)
        nxt += n

    # ---- queries
    H = hadamard()
    t0 = sdist = None
    if kind == "U":
        sign = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)  # one sign per dim
        sign[0] = 1.0  # q . poison K > 0
        q = torch.tensor(Q_VALUES)[torch.randint(0, 4, (T, hq, D), generator=g)] * sign
    else:
        tpw = max(1, 32 // G)  # tokens per 32-row tile of paged_attn_kernel<2>
        cl = torch.empty(T, hq, dtype=torch.int64)
        sdist = torch.empty(T, hq, dtype=torch.int64)
        row = 0
        for b, n in enumerate(q_lens):
            for i in range(n):
                L = lens[row]
                kv_end = prefix[b] + min(n, (i // tpw + 1) * tpw)
                cand = [0] + ([-1] if L > D else []) + [s for s in SWEEP[1:] if L - 1 - s >= 0]
                for p in _extras(L, prefix[b], kv_end, splits):
                    if L - 1 - p not in cand:
                        cand.append(L - 1 - p)
                rot = hq if hq < len(cand) else 1
                for hd in range(hq):
                    s = cand[(hd + rot * (n - 1 - i)) % len(cand)]  # the chunk's last token starts the sweep
                    sdist[row, hd] = s
                    cl[row, hd] = cls(L - 1 - s, hd // G)
                row += 1
        q = A_Q * H[cl]
        t0 = (cl - 3 * (torch.arange(hq) // G)[None, :]) % D
        assert bool((t0 < torch.tensor(lens)[:, None]).all()), "every row must see at least one key of its class"

    # ---- caches (logical f32): poison everywhere, then each sequence's valid tokens
    kc = torch.zeros(nb, hkv, bs, D)
    kc[..., 0] = POISON_K0
    vc = torch.full((nb, hkv, D, bs), POISON_V)
    codes = code_rows(MAX_CTX + 5 * hkv + 1)
    hk = torch.arange(hkv)
    for b, c in enumerate(ctx):
        blocks = bt[b, :nbs[b]].long()
        t = torch.arange(c)
        idx = t[:, None] + 5 * hk[None, :]  # [c, hkv]
        if kind == "U":
            K = torch.zeros(c, hkv, D)
            V = torch.nn.functional.one_hot(idx % D, D).float()
        else:
            K = B_K * H[cls(t[:, None], hk[None, :])]
            V = codes[idx]
        kc[blocks[t // bs], :, t % bs] = K
        vc[blocks[t // bs], :, :, t % bs] = V
    ks, vs = (K_SCALE, V_SCALE) if fp8 else (1.0, 1.0)
    k, v = _store(kc, fp8, ks), _store(vc, fp8, vs)

    # ---- closed form
    expect = torch.empty(T, hq, D)
    Lt = torch.tensor(lens)
    if kind == "U":
        for row, L in enumerate(lens):
            for h in range(hkv):
                expect[row, h * G:(h + 1) * G] = (u_counts(L, h).double() / L).float()
    else:
        nmax = (MAX_CTX + D - 1) // D
        for h in range(hkv):
            pos = torch.arange(D)[:, None] + D * torch.arange(nmax)[None, :] + 5 * h  # [t0, j]
            cs = codes[pos.clamp(max=codes.shape[0] - 1)].double().cumsum(1)  # [t0, j, 128]
            tt = t0[:, h * G:(h + 1) * G]
            n = (Lt[:, None] - tt + D - 1) // D  # members t0 + 128 j < L
            assert int(n.min()) >= 1 and int((tt + D * (n - 1) + 5 * h).max()) < codes.shape[0]
            expect[:, h * G:(h + 1) * G] = (cs[tt, n - 1] / n[..., None]).float()
    return Probe(kind, hq, hkv, bs, fp8, _store(q, False), k, v, bt, torch.tensor(qs, dtype=torch.int32),
                 torch.tensor(ctx, dtype=torch.int32), q_lens, prefix, lens, expect, t0, sdist, pad)


# ---- checks -------------------------------------------------------------------------------------------------------
def reference(p: Probe, *, ctx=None, k=None, v=None, bt=None) -> torch.Tensor:
    """The project's fp32 reference on the probe (optionally on mutated inputs); q is passed as f32 (it is exact in
    bf16), so the output is not rounded to bf16."""
    ks, vs = p.scales
    return ref.paged_attention(p.q.float(), p.k if k is None else k, p.v if v is None else v,
                               p.bt if bt is None else bt, p.qs, p.ctx if ctx is None else ctx,
                               torch.zeros(1, 2, dtype=torch.int32), 1, 8, 1, None, ks, vs)


def bound(p: Probe) -> torch.Tensor:
    e = p.expect.abs()
    return U_REL * e + U_ABS if p.kind == "U" else N_REL * e + N_ABS


def excess(out: torch.Tensor, p: Probe) -> torch.Tensor:
    """[T, hq]: the largest |out - e| / bound over the row's dims (inf where not finite); > 1 is a violation."""
    o = out.float().cpu()
    r = ((o - p.expect) / bound(p)).abs()
    return torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf"))).amax(-1)


def violations(out: torch.Tensor, p: Probe) -> torch.Tensor:
    """bool [T, hq]: rows outside the bound (or not finite)."""
    return ~(excess(out, p) <= 1.0)


def members(p: Probe, row: int, hd: int) -> list:
    return list(range(int(p.t0[row, hd]), p.lens[row], D))


def signature(out: torch.Tensor, p: Probe, limit: int = 6) -> str:
    """Which keys a failing output points at.  U: the dims that are off and by how many counts (out * L - count).
    C: which class member is missing, extra or exchanged, solved from out * n' - sum over the row's members for
    n' = n - 1, n + 1 and n (the hypothesis with the smallest residual is named)."""
    o = out.float().cpu()
    bad = violations(o, p).nonzero().tolist()
    G = p.hq // p.hkv
    seq_of = p.seq_of
    lines = [f"{len(bad)} of {o.shape[0] * o.shape[1]} (token, head) rows off"]
    codes = code_rows(MAX_CTX + 5 * p.hkv + 1).double()
    for row, hd in bad[:limit]:
        L, h, b = p.lens[row], hd // G, seq_of[row]
        head = f"seq {b} ctx {int(p.ctx[b])} token {row - int(p.qs[b])} head {hd} L {L}: "
        x = o[row, hd].double()
        if not bool(torch.isfinite(x).all()):
            lines.append(head + "non-finite output")
        elif p.kind == "U":
            delta = (x * L - u_counts(L, h)).round().long()
            dims = delta.nonzero().flatten().tolist()
            lines.append(head + "count deltas " + ", ".join(f"d{d} (key {(d - 5 * h) % D} mod 128): {int(delta[d]):+d}"
                                                            for d in dims[:8]) + f" [{len(dims)} dims]")
        else:
            mem = members(p, row, hd)
            n, S = len(mem), codes[torch.tensor(mem) + 5 * h].sum(0)
            hyp = []
            for m in mem:  # one member missing: out (n - 1) = S - v_m
                if n > 1:
                    hyp.append((float((x * (n - 1) - S + codes[m + 5 * h]).abs().max()), f"member {m} missing"))
            res = (codes[5 * h:] - (x * (n + 1) - S)[None]).abs().amax(-1)  # one key extra: out (n + 1) = S + v_x
            t = int(res.argmin())
            hyp.append((float(res[t]), f"key {t} extra"))
            hyp.append((float((x * (n + 1) - S - POISON_V).abs().max()), "a poison slot extra"))
            for m in mem:  # V of member m exchanged for another key's: out n = S - v_m + v_x
                res = (codes[5 * h:] - (x * n - S + codes[m + 5 * h])[None]).abs().amax(-1)
                t = int(res.argmin())
                hyp.append((float(res[t]), f"member {m} returned the V of key {t}"))
            r, what = min(hyp)
            if r > 0.25:
                what = f"no one-key explanation (the nearest: {what})"
            err = float((x - p.expect[row, hd]).abs().max())
            lines.append(head + f"class {int(cls(mem[0], h))} members {mem[:3]}..{mem[-1]} (n {n}, aimed at s "
                                f"{int(p.sdist[row, hd])}): {what} (residual {r:.3g}), max err {err:.4g}")
    return "\n".join(lines)


def check(out: torch.Tensor, p: Probe, what: str = "") -> None:
    assert not bool(violations(out, p).any()), f"{what} {p.kind} probe: " + signature(out, p)


def margin_log2(p: Probe) -> float:
    """C probe, fp64 from the stored tensors (after fp8 dequantisation): asserts that every key outside a row's class
    scores exactly 0 and returns the smallest lead, in log2 units, of a row's class members over the others."""
    G, worst = p.hq // p.hkv, float("inf")
    ks, _ = p.scales
    row = 0
    for b, n in enumerate(p.q_lens):
        c = int(p.ctx[b])
        blocks = p.bt[b, :(c + p.bs - 1) // p.bs].long()
        K = _load(p.k[blocks], p.fp8, ks).double().permute(1, 0, 2, 3).reshape(p.hkv, -1, D)[:, :c]
        for i in range(n):
            L = p.lens[row]
            s = torch.einsum("hgd,hkd->hgk", p.q[row].double().view(p.hkv, G, D), K[:, :L]) * (LOG2E / math.sqrt(D))
            mine = (torch.arange(L)[None, None, :] - p.t0[row].view(p.hkv, G, 1)) % D == 0
            assert bool((s[~mine] == 0).all()), "a key outside the class must score exactly 0"
            worst = min(worst, float(s[mine].min()))
            row += 1
    return worst


def holds(p: Probe, pos: int, seq: int | None = None) -> torch.Tensor:
    """bool [T, hq]: rows (of sequence ``seq``) whose class has a visible member at position ``pos``."""
    Lt = torch.tensor(p.lens)[:, None]
    m = (pos < Lt) & ((pos - p.t0) % D == 0) & (pos >= 0)
    if seq is not None:
        m &= (torch.tensor(p.seq_of) == seq)[:, None]
    return m


def waves(p: Probe) -> torch.Tensor:
    """[T, hq]: the wave of a flash-prefill tile (128 rows, token-major, 32 per wave) that owns the row."""
    G = p.hq // p.hkv
    tpw = 128 // G
    i = torch.cat([torch.arange(n) for n in p.q_lens])
    return ((i % tpw)[:, None] * G + (torch.arange(p.hq) % G)[None, :]) // 32


# ---- mutations of the reference's inputs: the probes must notice each ---------------------------------------------
# each returns (kwargs for ``reference``, ok: the sequences it applies to, must: bool [T, hq] rows that must be flagged,
# exact: whether no other row may be flagged)
def _rows(p: Probe, ok) -> torch.Tensor:
    return torch.tensor([ok[b] for b in p.seq_of])[:, None].expand(-1, p.hq)


def mutate_drop_last(p: Probe):
    """Every context one key shorter (sequences whose every row keeps at least one key): every row loses its diagonal
    key.  U: every row moves.  C: exactly the rows whose class is the diagonal key's."""
    ok = [pre >= 1 for pre in p.prefix]
    ctx = p.ctx - torch.tensor(ok, dtype=torch.int32)
    Lt = torch.tensor(p.lens)[:, None]
    must = _rows(p, ok) & (True if p.kind == "U" else (Lt - 1 - p.t0) % D == 0)
    return dict(ctx=ctx), ok, must, True


def mutate_read_past(p: Probe):
    """ctx_len + 1 where the last page has a free slot: every row sees the key after its diagonal — the next token's
    for all but the chunk's last token, whose extra key is the poison slot.  U: every row moves.  C: the rows whose
    class is that of the first masked key, and every head of the last token."""
    ok = [int(c) % p.bs != 0 for c in p.ctx.tolist()]
    ctx = p.ctx + torch.tensor(ok, dtype=torch.int32)
    Lt = torch.tensor(p.lens)[:, None]
    last = torch.zeros(len(p.lens), dtype=torch.bool)
    last[p.qs[1:].long() - 1] = True
    must = _rows(p, ok) & (True if p.kind == "U" else ((Lt - p.t0) % D == 0) | last[:, None])
    return dict(ctx=ctx), ok, must, True


def _seq_member(p: Probe, b: int, want) -> int | None:
    """A visible member position t of some row of sequence b with want(t), the latest row first."""
    if p.kind == "U":
        cand = range(int(p.ctx[b]) - 1, -1, -1)
        return next((t for t in cand if want(t)), None)
    for row in range(int(p.qs[b + 1]) - 1, int(p.qs[b]) - 1, -1):
        for hd in range(p.hq):
            for t in reversed(members(p, row, hd)):
                if want(t):
                    return t
    return None


def _swap_must(p: Probe, b: int, t: int, u: int, which: str) -> torch.Tensor:
    """Rows of sequence b that an exchange of (V | K) between positions t and u moves."""
    Lt = torch.tensor(p.lens)[:, None]
    seq = (torch.tensor(p.seq_of) == b)[:, None]
    if p.kind == "U":  # a uniform average sees an exchange of V only where exactly one of the two is visible
        if which == "k":
            return torch.zeros(len(p.lens), p.hq, dtype=torch.bool)
        return (seq & ((t < Lt) != (u < Lt))).expand(-1, p.hq)
    mt, mu = (t - p.t0) % D == 0, (u - p.t0) % D == 0  # rows of t's / u's class (t, u < 128 apart: never both)
    if which == "v":  # a member's V is another key's as soon as the member is visible
        return seq & ((mt & (t < Lt)) | (mu & (u < Lt)))
    # K exchanged, V in place: the class of t now sits at u and the other way round
    return seq & ((mt | mu) & ((t < Lt) | (u < Lt)))


def mutate_swap_v(p: Probe):
    """Per sequence, V of two neighbouring tokens (t, t ^ 1) exchanged, t a class member of one of its rows."""
    v = p.v.clone()
    ok, must = [], torch.zeros(len(p.lens), p.hq, dtype=torch.bool)
    for b, c in enumerate(p.ctx.tolist()):
        t = _seq_member(p, b, lambda t: (t ^ 1) < c)
        ok.append(t is not None)
        if t is None:
            continue
        u = t ^ 1
        bt_, bu = int(p.bt[b, t // p.bs]), int(p.bt[b, u // p.bs])
        a = v[bt_, :, :, t % p.bs].clone()
        v[bt_, :, :, t % p.bs] = v[bu, :, :, u % p.bs]
        v[bu, :, :, u % p.bs] = a
        must |= _swap_must(p, b, t, u, "v")
    return dict(v=v), ok, must, True


def mutate_swap_k(p: Probe):
    """Per sequence, K of two tokens of one 16-key page exchanged with V left in place; the two positions differ
    exactly in bits 2 and 3 (t ^ 12 with t % 16 in 4..11), the pair the fp8-MFMA kernels' ``kperm`` exchanges.
    U (K = 0 everywhere) cannot see it."""
    k = p.k.clone()
    ok, must = [], torch.zeros(len(p.lens), p.hq, dtype=torch.bool)
    for b, c in enumerate(p.ctx.tolist()):
        t = _seq_member(p, b, lambda t: 4 <= t % 16 < 12 and (t ^ 12) < c)
        ok.append(t is not None)
        if t is None:
            continue
        u = t ^ 12
        assert t // 16 == u // 16 and bin(t ^ u) == "0b1100"
        blk = int(p.bt[b, t // p.bs])
        a = k[blk, :, t % p.bs].clone()
        k[blk, :, t % p.bs] = k[blk, :, u % p.bs]
        k[blk, :, u % p.bs] = a
        must |= _swap_must(p, b, t, u, "k")
    return dict(k=k), ok, must, True


def mutate_shift_table(p: Probe):
    """Every block table shifted by one entry (entry i <- entry i + 1, the last <- the padding block).  K and V move
    together, so the comb sees the page that fell off the front (rows whose class starts inside it) and the poison page
    at the end (every row that reaches the sequence's last page); U counts other positions in every row."""
    bt = torch.cat([p.bt[:, 1:], torch.full((p.B, 1), p.pad, dtype=torch.int32)], dim=1)
    ok = [True] * p.B
    Lt = torch.tensor(p.lens)[:, None]
    last_page = torch.tensor([(int(p.ctx[b]) - 1) // p.bs * p.bs for b in p.seq_of])[:, None]
    if p.kind == "U":  # the window [bs, L + bs) counts like [0, L) only where L is a multiple of 128
        must = ((Lt % D != 0) | (Lt > last_page)).expand(-1, p.hq)
    else:
        must = (p.t0 < p.bs) | (Lt > last_page)
    return dict(bt=bt), ok, must, False


MUTATIONS = {"drop_last": mutate_drop_last, "read_past": mutate_read_past, "swap_v": mutate_swap_v,
             "swap_k": mutate_swap_k, "shift_table": mutate_shift_table}


# ---- the shapes the GPU tests launch (tests/test_prefill_probes_gpu.py), also walked by the CPU tests ----------------
# a one-token sequence and a fresh prompt; prefixes that are no multiple of 16 or 64; partial last pages and partial
# last tiles at every G; several tiles per sequence; one context past the 1024-token window
RAGGED = dict(q_lens=[1, 17, 64, 5, 100, 33], prefix=[0, 0, 136, 32, 0, 1100])
# G = 1: 128 tokens per tile, a last tile with two valid rows, a wave_min_pos per wave
G1 = dict(q_lens=[130, 40], prefix=[300, 5], hq=4, hkv=4)
SHAPES = {
    # id: (build kwargs, kinds)
    "ragged32x8": (dict(RAGGED, hq=32, hkv=8, seed=41), "UC"),
    "ragged64x8": (dict(RAGGED, hq=64, hkv=8, seed=42), "UC"),
    "ragged16x1": (dict(RAGGED, hq=16, hkv=1, seed=43), "UC"),
    "ragged4x4": (dict(RAGGED, hq=4, hkv=4, seed=44), "UC"),
    "ragged12x3": (dict(RAGGED, hq=12, hkv=3, seed=45), "UC"),  # hkv no power of two: no fp8-MFMA kernel
    "g1_two_tiles": (dict(G1, seed=46), "UC"),
    "long_u": (dict(q_lens=[200], prefix=[2000], hq=32, hkv=8, width=144, seed=47), "U"),
    "ragged32x8_p32": (dict(RAGGED, hq=32, hkv=8, bs=32, seed=48), "UC"),
    "ragged16x1_p32": (dict(RAGGED, hq=16, hkv=1, bs=32, seed=49), "UC"),
    "g1_two_tiles_p32": (dict(G1, bs=32, seed=50), "UC"),
    "ragged32x8_split": (dict(RAGGED, hq=32, hkv=8, splits=True, seed=51), "UC"),
    "ragged4x4_split": (dict(RAGGED, hq=4, hkv=4, splits=True, seed=52), "UC"),
    "ragged16x1_split": (dict(RAGGED, hq=16, hkv=1, splits=True, seed=53), "UC"),
    "ragged32x8_p32_split": (dict(RAGGED, hq=32, hkv=8, bs=32, splits=True, seed=54), "UC"),
}


@functools.lru_cache(maxsize=None)
def probe(shape: str, kind: str, fp8: bool = False) -> Probe:
    """The CPU probe of a GPU test shape (built once per process)."""
    kw, kinds = SHAPES[shape]
    assert kind in kinds
    return build(kind, fp8=fp8, **kw)
