"""Exact per-key probes for decode attention (csrc/kernels/attention.hip: paged_decode_kernel, split_decode_kernel,
paged_attn_kernel<1>, casc_prefix_kernel), shared by tests/test_decode_probes.py (CPU: builders, closed forms and
mutation checks against chronos.ops.reference) and tests/test_decode_probes_gpu.py (the HIP kernels).

Random K / V under ``atol 2e-2`` cannot see one dropped, doubled, stale or mis-paired key: with the softmax weight
spread over ctx keys a single wrong key moves the output by about |v| / ctx.  The probes here have closed-form outputs
in which one wrong key is a large, attributable error.  Page size 16, D = 128, block ids randomly permuted; every stored
value is exact in bf16 AND in e4m3 at the power-of-two cache scale 0.5, so the same probe serves bf16 and fp8 KV.

U (uniform) — which keys are attended.  K = 0 at every valid position, so every score is 0 and the softmax is exactly
    uniform; V[h][t, d] = 1 if d == (t + 5 h) % 128 else 0; q random (it must not matter).  Expected output of (any q
    head of kv head h, dim d) = count[h, d] / L with count the number of t < L hitting d (integer arithmetic) and L the
    row's causal length (ctx for one-token decode, ctx - (n - 1 - j) for token j of an n-token chunk).
N (needle) — which V goes with which K.  MFMA column c = token j * G + head g of a sequence carries q = 4.0 on the
    eight dims {4c..4c+3} U {64+4c..64+4c+3} (closed under the rotate-half pairing, so the supports stay disjoint after
    RoPE); its needle key at position p equals 4 q (needles sharing a position are summed): score 4 * 128 / sqrt(128) =
    45.3 nat = 65 log2 units against 0 everywhere else.  V[h][t, :] is the position code ``code_rows`` of t + 5 h.
    Expected output = the code row of p; ``margin_log2`` proves the leak is below ctx * 2^-30.

Poison (both probes): every cache block outside all block tables (the table padding points at one), every slot at or
past ctx in a sequence's last block and — fused RoPE probes — the new token's slot before the call hold K = 4 q of
the sequence's first q head of the kv head and V = 64.0, finite: a read past the context, of a stale slot or through a
wrong table entry swamps the output, a masked read contributes exactly 0.

Tolerances (derived, not measured).  p = 2^0 and l = L are exact in fp32 and O is an exact integer (U) / one code row
plus a leak below L * 2^-30 (N).  The only roundings are the round-to-nearest bf16 store of the output (8 significant
bits: at most 2^-8 relative) and, under the cascade, the producer's bf16 O (another 2^-8 at most, weighted by the
prefix's share of the softmax, which is below 1 because a member has at least one key past the prefix) — together
strictly inside 2^-7; the split combine's 1 / L and exp2 / log2 add a few 2^-22.  N's code rows are bf16 numbers, so a
correct kernel returns them exactly.
    U: |out - count / L| <= 2^-7 * count / L + 1e-6     (L <= 4096 -> count <= 32: one wrong key is >= 1/32 relative,
                                                         four times the bound; count = 0 dims are 0 within 1e-6)
    N: |out - V[p]|      <= 2^-7 * |V[p]| + 2^-7        (two code rows differ by >= 0.5 in most dims)
"""
from __future__ import annotations

import dataclasses
import functools
import math

import torch

from chronos.ops import reference as ref

D, BS = 128, 16
KV_SCALE = 0.5  # fp8 k_scale = v_scale (a power of two: dequantisation is exact)
POISON_V = 64.0
Q_VALUES = (0.5, 1.0, 1.5, 2.0)  # U probe |q| entries: 4 q / KV_SCALE <= 16 is exact in e4m3
MODULI = ((29, 43), (31, 43), (33, 42))  # (modulus, dims): pairwise coprime, product 29667 > 4096 + 5 * 63
U_REL, U_ABS = 2.0 ** -7, 1e-6
N_REL, N_ABS = 2.0 ** -7, 2.0 ** -7
LOG2E = 1.4426950408889634


def code_rows(n: int) -> torch.Tensor:
    """[n, 128] f32 position code: over the dims of modulus m, dim k holds ((t % m + k) % m) % 16 - 7.5 —
    half-integers with |v| <= 7.5 (exact in bf16, and in e4m3 at scale 0.5).  Two residues r1 != r2 of an odd m differ
    at every k where exactly one of r + k wraps (their difference is d or d - m there, not both multiples of 16), and
    each range spans a whole period, so by the CRT no two t below 29 * 31 * 33 share a row."""
    t = torch.arange(n)
    out = torch.empty(n, D)
    lo = 0
    for m, w in MODULI:
        k = torch.arange(w)
        out[:, lo:lo + w] = (((t[:, None] % m) + k[None, :]) % m % 16).float() - 7.5
        lo += w
    return out


def u_counts(L: int, h: int) -> torch.Tensor:
    """int64 [128]: number of t in [0, L) with (t + 5 h) % 128 == d."""
    r = (torch.arange(D) - 5 * h) % D  # the first t hitting dim d
    return torch.clamp((L - r + D - 1) // D, min=0)


@dataclasses.dataclass
class Probe:
    kind: str  # "U" | "N"
    hq: int
    hkv: int
    fp8: bool
    q: torch.Tensor  # [T, hq, 128] bf16: the queries of paged_attention (fused RoPE probes: the reference-roped q)
    k: torch.Tensor  # caches the attention reads (fused RoPE probes: after the reference rope_kv_write)
    v: torch.Tensor
    bt: torch.Tensor  # [B, W] int32, padded with the id of a poison block
    qs: torch.Tensor  # [B + 1] int32
    ctx: torch.Tensor  # [B] int32
    q_lens: list
    lens: list  # causal length of every query row (token)
    expect: torch.Tensor  # [T, hq, 128] f32 closed form
    needle: torch.Tensor | None  # [T, hq] int64 needle position (N)
    pad: int  # the poison block the table padding points at
    # fused RoPE probes (ops.decode_attention_rope)
    qkv: torch.Tensor | None = None  # [B, (hq + 2 hkv) * 128] bf16 raw projection
    pos: torch.Tensor | None = None
    cos_sin: torch.Tensor | None = None
    k_pre: torch.Tensor | None = None  # caches before the call: the new token's slot poisoned
    v_pre: torch.Tensor | None = None
    casc: list | None = None  # shared prefix block ids (cascade probes)

    @property
    def B(self) -> int:
        return len(self.q_lens)

    @property
    def max_q(self) -> int:
        return max(self.q_lens)

    @property
    def scales(self):
        return (KV_SCALE, KV_SCALE) if self.fp8 else (1.0, 1.0)

    def to(self, dev) -> "Probe":
        kw = {f.name: (getattr(self, f.name).to(dev) if isinstance(getattr(self, f.name), torch.Tensor)
                       else getattr(self, f.name)) for f in dataclasses.fields(self)}
        return Probe(**kw)


def _store(x: torch.Tensor, fp8: bool, scale: float = KV_SCALE) -> torch.Tensor:
    """Logical f32 cache -> stored bf16 / e4m3 bytes (value / scale); the probes must survive it unchanged."""
    if fp8:
        b = (x / scale).to(torch.float8_e4m3fn)
        assert torch.equal(b.float() * scale, x), "probe value not exact in e4m3"
        return b.view(torch.uint8)
    b = x.to(torch.bfloat16)
    assert torch.equal(b.float(), x), "probe value not exact in bf16"
    return b


def _load(x: torch.Tensor, fp8: bool, scale: float = KV_SCALE) -> torch.Tensor:
    return ref.from_fp8_bytes(x, scale) if fp8 else x.float()


def _q_support(c: int) -> list:
    return list(range(4 * c, 4 * c + 4)) + list(range(64 + 4 * c, 64 + 4 * c + 4))


def _dedup(xs, L):
    out = []
    for p in xs:
        if 0 <= p < L and p not in out:
            out.append(p)
    return out


def split_edges(ctx: int, nsplits=(16, 4, 3, 2)) -> list:
    """First and last keys of the kv splits of a ctx-token context (chunk = ceil(ctx / nsplit) rounded up to 32, as
    the kernels cut it), round-robin over the split counts so a short list still names every count."""
    per = []
    for ns in nsplits:
        chunk = ((ctx + ns - 1) // ns + 31) & ~31
        per.append([p for e in range(chunk, ctx, chunk) for p in (e - 1, e)])
    out = []
    for i in range(max((len(x) for x in per), default=0)):
        out += [x[i] for x in per if i < len(x)]
    return out


def default_needles(ctx, q_lens, hq, g, *, splits=False, prefix=0, phase=0) -> torch.Tensor:
    """[T, hq] needle positions.  Every third sequence sweeps the 32 slots of one 32-token step over its heads (slot
    (head + hq * b / 3) % 32 of the second step or, alternately, of the last full step); the others take, in head order,
    the first key, the last key, (the first and last keys of the kv splits,) both sides of the 32 / 64-token step
    edges and of the 1024-token block-table window, then random positions.  Cascade (prefix = P blocks): heads of parity
    ``phase`` of a member sequence share one needle inside the prefix (a function of the head alone: the prefix K is
    shared), the others start at the first token past it."""
    rows = []
    for b, (c, n) in enumerate(zip(ctx, q_lens)):
        member = prefix > 0 and c > BS * prefix
        lo = BS * prefix if member else 0
        for i in range(n):
            L = c - (n - 1 - i)
            cand = [lo, L - 1] + (split_edges(c) if splits else [])
            cand += [lo + 1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, L - 2, 15, 16, 17]
            cand = [p for p in _dedup(cand, L) if p >= lo]
            row = []
            for hd in range(hq):
                if member and hd % 2 == phase:
                    shared = [0, BS * prefix - 1, 15, 16, BS * prefix - 2]
                    row.append((shared[hd // 2] if hd // 2 < len(shared) else 7 * hd + 3) % (BS * prefix))
                elif b % 3 == 1 and L - lo >= 32:
                    steps = (L - lo) // 32
                    s = lo + 32 * ((steps - 1) if (b // 3) % 2 else min(1, steps - 1))
                    row.append(s + (hd + hq * (b // 3)) % 32)
                elif hd < len(cand):
                    row.append(cand[(hd + (hq * (b // 3) if hq < 16 else 0)) % len(cand)])
                else:
                    row.append(lo + int(torch.randint(0, L - lo, (1,), generator=g)))
            rows.append(row)
    return torch.tensor(rows, dtype=torch.int64)


def build(kind: str, ctx, hq: int, hkv: int, *, q_lens=None, fp8: bool = False, seed: int = 0, width: int | None = None,
          needles: torch.Tensor | None = None, splits: bool = False, rope: torch.Tensor | None = None,
          prefix: int = 0, phase: int = 0) -> Probe:
    """One launch's probe on the CPU.  ``rope``: a cos_sin table -> a fused RoPE + KV-write probe (one token per
    sequence, bf16).  ``prefix``: P shared leading blocks held by every sequence with ctx > 16 P (cascade)."""
    assert kind in ("U", "N") and max(ctx) <= 4096 and not (rope is not None and fp8)
    g = torch.Generator().manual_seed(seed)
    B, G = len(ctx), hq // hkv
    q_lens = list(q_lens) if q_lens is not None else [1] * B
    assert rope is None or max(q_lens) == 1
    T = sum(q_lens)
    qs = [0]
    for n in q_lens:
        qs.append(qs[-1] + n)
    lens = [c - (n - 1 - i) for c, n in zip(ctx, q_lens) for i in range(n)]
    assert min(lens) >= 1 and max(q_lens) * G <= 16

    # ---- block tables: randomly permuted ids, the prefix blocks shared, the padding -> a poison block
    nbs = [(c + BS - 1) // BS for c in ctx]
    member = [prefix > 0 and c > BS * prefix for c in ctx]
    owned = prefix + sum(n - (prefix if m else 0) for n, m in zip(nbs, member))
    nb = owned + 3
    perm = torch.randperm(nb, generator=g).tolist()
    shared, nxt, pad = perm[:prefix], prefix, perm[-1]
    W = width if width is not None else max(nbs)
    assert W >= max(nbs)
    bt = torch.full((B, W), pad, dtype=torch.int32)
    for b, (n, m) in enumerate(zip(nbs, member)):
        ids = (shared if m else []) + perm[nxt:nxt + n - (prefix if m else 0)]
        nxt += n - (prefix if m else 0)
        bt[b, :n] = torch.tensor(ids, dtype=torch.int32)
    assert nxt == owned

    # ---- queries (raw); column c = token i * G + head g of the kv head's MFMA tile
    if kind == "U":
        sign = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)  # one sign per dim: q . poison K > 0
        q_raw = torch.tensor(Q_VALUES)[torch.randint(0, 4, (T, hq, D), generator=g)] * sign
    else:
        q_raw = torch.zeros(T, hq, D)
        for b, n in enumerate(q_lens):
            for i in range(n):
                for hd in range(hq):
                    q_raw[qs[b] + i, hd, _q_support(i * G + hd % G)] = 4.0
        if needles is None:
            needles = default_needles(ctx, q_lens, hq, g, splits=splits, prefix=prefix, phase=phase)
        assert needles.shape == (T, hq) and bool((needles >= 0).all())
        assert bool((needles < torch.tensor(lens)[:, None]).all()), "a needle must be a key its row may attend"
    pos = torch.tensor(ctx, dtype=torch.int32) - 1
    tok = torch.arange(B, dtype=torch.int32)
    if rope is not None:  # the reference's roped q: what the keys must match
        qkv0 = torch.zeros(B, hq + 2 * hkv, D)
        qkv0[:, :hq] = q_raw
        qk = torch.empty(B, hq, D, dtype=torch.bfloat16)
        ref.rope_kv_write(qkv0.to(torch.bfloat16).view(B, -1), pos, tok, bt, rope, qk,
                          torch.zeros(nb, hkv, BS, D, dtype=torch.bfloat16),
                          torch.zeros(nb, hkv, D, BS, dtype=torch.bfloat16), hq, hkv)
        qk = qk.float()
    else:
        qk = q_raw

    # ---- caches (logical f32): poison everywhere, then each sequence's valid tokens
    heads0 = torch.arange(hkv) * G  # first q head of every kv head
    kc = (4.0 * qk[0, heads0])[None, :, None, :].repeat(nb, 1, BS, 1)
    vc = torch.full((nb, hkv, D, BS), POISON_V)
    codes = code_rows(4096 + 5 * hkv + 1)
    hk = torch.arange(hkv)
    k_new = torch.zeros(B, hkv, D)  # fused RoPE: the raw K row of the new token (needles at the new token)
    done_prefix = False
    for b, c in enumerate(ctx):
        blocks = bt[b, :nbs[b]].long()
        own = blocks[prefix:] if member[b] else blocks
        kc[own] = (4.0 * qk[qs[b], heads0])[None, :, None, :]
        nt = c - 1 if rope is not None else c  # fused RoPE: the new token's slot stays poisoned before the call
        t = torch.arange(nt)
        K = torch.zeros(nt, hkv, D)
        idx = t[:, None] + 5 * hk[None, :]  # [nt, hkv]
        V = torch.nn.functional.one_hot(idx % D, D).float() if kind == "U" else codes[idx]
        if kind == "N":
            for i in range(q_lens[b]):
                for hd in range(hq):
                    p = int(needles[qs[b] + i, hd])
                    if p < nt:
                        K[p, hd // G] += 4.0 * qk[qs[b] + i, hd]
                    else:  # the new token: raw k = 4 raw q (RoPE at equal positions preserves the dot product)
                        k_new[b, hd // G] += 4.0 * q_raw[qs[b] + i, hd]
        if member[b] and done_prefix:  # the shared blocks are written once; every member must agree on them
            n0 = BS * prefix
            assert torch.equal(kc[blocks[t[:n0] // BS], :, t[:n0] % BS], K[:n0]), "members disagree on the prefix K"
            t, K, V = t[n0:], K[n0:], V[n0:]
        done_prefix = done_prefix or member[b]
        kc[blocks[t // BS], :, t % BS] = K
        vc[blocks[t // BS], :, :, t % BS] = V
    k, v = _store(kc, fp8), _store(vc, fp8)

    # ---- closed form
    expect = torch.empty(T, hq, D)
    for row, L in enumerate(lens):
        for h in range(hkv):
            if kind == "U":
                expect[row, h * G:(h + 1) * G] = (u_counts(L, h).double() / L).float()
            else:
                expect[row, h * G:(h + 1) * G] = codes[needles[row, h * G:(h + 1) * G] + 5 * h]
    p = Probe(kind, hq, hkv, fp8, qk.to(torch.bfloat16), k, v, bt, torch.tensor(qs, dtype=torch.int32),
              torch.tensor(ctx, dtype=torch.int32), q_lens, lens, expect, needles, pad)
    if rope is None:
        return p
    qkv = torch.zeros(B, hq + 2 * hkv, D)
    qkv[:, :hq] = q_raw
    qkv[:, hq:hq + hkv] = k_new
    idx = pos.long()[:, None] + 5 * hk[None, :]
    qkv[:, hq + hkv:] = torch.nn.functional.one_hot(idx % D, D).float() if kind == "U" else codes[idx]
    p.qkv = _store(qkv, False).view(B, -1)
    p.pos, p.cos_sin, p.k_pre, p.v_pre, p.casc = pos, rope, k, v, shared
    p.k, p.v = k.clone(), v.clone()
    q2 = torch.empty(B, hq, D, dtype=torch.bfloat16)
    ref.rope_kv_write(p.qkv, pos, tok, bt, rope, q2, p.k, p.v, hq, hkv)
    assert torch.equal(q2, p.q)
    return p


# ---- checks -------------------------------------------------------------------------------------------------------
def reference(p: Probe, *, ctx=None, v=None, bt=None) -> torch.Tensor:
    """The project's fp32 reference on the probe (optionally on mutated inputs); q is passed as f32 (it is exact in
    bf16), so the output is not rounded to bf16."""
    ks, vs = p.scales
    return ref.paged_attention(p.q.float(), p.k, p.v if v is None else v, p.bt if bt is None else bt, p.qs,
                               p.ctx if ctx is None else ctx, None, p.B, 1, 1, None, ks, vs, max_q=p.max_q)


def bound(p: Probe) -> torch.Tensor:
    e = p.expect.abs()
    return U_REL * e + U_ABS if p.kind == "U" else N_REL * e + N_ABS


def violations(out: torch.Tensor, p: Probe, tol: torch.Tensor | None = None) -> torch.Tensor:
    """bool [T, hq]: rows outside the bound (or not finite)."""
    o = out.float().cpu()
    e = p.expect.cpu()
    tol = bound(p).cpu() if tol is None else tol
    return (~((o - e).abs() <= tol)).any(-1)


def signature(out: torch.Tensor, p: Probe, limit: int = 6) -> str:
    """Which keys a failing output points at.  U: the dims that are off and by how many counts (out * L - count).
    N: the position whose code row came back (nearest row) against the needle."""
    o = out.float().cpu()
    bad = violations(o, p).nonzero().tolist()
    G = p.hq // p.hkv
    seq_of = [b for b, n in enumerate(p.q_lens) for _ in range(n)]
    lines = [f"{len(bad)} of {o.shape[0] * o.shape[1]} (token, head) rows off"]
    codes = code_rows(4096 + 5 * p.hkv + 1)
    for row, hd in bad[:limit]:
        L, h = p.lens[row], hd // G
        head = f"seq {seq_of[row]} ctx {int(p.ctx[seq_of[row]])} row {row} head {hd} L {L}: "
        if not bool(torch.isfinite(o[row, hd]).all()):
            lines.append(head + "non-finite output")
        elif p.kind == "U":
            delta = (o[row, hd].double() * L - u_counts(L, h)).round().long()
            dims = delta.nonzero().flatten().tolist()
            lines.append(head + "count deltas " + ", ".join(f"d{d} (key {(d - 5 * h) % D} mod 128): {int(delta[d]):+d}"
                                                            for d in dims[:8]) + f" [{len(dims)} dims]")
        else:
            near = int((codes - o[row, hd][None]).abs().sum(-1).argmin()) - 5 * h
            err = float((o[row, hd] - p.expect[row, hd]).abs().max())
            lines.append(head + f"needle at {int(p.needle[row, hd])}, nearest code row is position {near}, "
                                f"max err {err:.4g}")
    return "\n".join(lines)


def check(out: torch.Tensor, p: Probe, what: str = "") -> None:
    assert not bool(violations(out, p).any()), f"{what} {p.kind} probe: " + signature(out, p)


def margin_log2(p: Probe) -> float:
    """N probe, fp64 from the stored tensors (after fp8 dequantisation / after RoPE): the smallest lead, in log2 units,
    of a row's needle score over every other key it may attend."""
    G, worst = p.hq // p.hkv, float("inf")
    row = 0
    for b, n in enumerate(p.q_lens):
        c = int(p.ctx[b])
        blocks = p.bt[b, :(c + BS - 1) // BS].long()
        K = _load(p.k[blocks], p.fp8).double().permute(1, 0, 2, 3).reshape(p.hkv, -1, D)[:, :c]
        for i in range(n):
            L = p.lens[row]
            s = torch.einsum("hgd,hkd->hgk", p.q[row].double().view(p.hkv, G, D), K[:, :L]) * (LOG2E / math.sqrt(D))
            nd = p.needle[row].view(p.hkv, G, 1)
            top = s.gather(-1, nd)
            rest = s.scatter(-1, nd, float("-inf")).amax(-1, keepdim=True)
            if L > 1:
                worst = min(worst, float((top - rest).min()))
            assert float(top.min()) > 30.0
            row += 1
    return worst


def coverage(p: Probe) -> dict:
    """Which of the required needle positions one launch's N probe holds."""
    first = last = False
    slots = {}
    allp = set()
    per_seq = [set() for _ in p.q_lens]
    seq_of = [b for b, n in enumerate(p.q_lens) for _ in range(n)]
    for row, L in enumerate(p.lens):
        for x in p.needle[row].tolist():
            first |= x == 0
            last |= x == L - 1
            allp.add(x)
            per_seq[seq_of[row]].add(x)
            slots.setdefault(x // 32, set()).add(x % 32)
    return {"first": first, "last": last, "step_slots": any(len(s) == 32 for s in slots.values()),
            "step_edge": {31, 32, 33} <= allp, "window": {1023, 1024, 1025} <= allp, "positions": allp,
            "per_seq": per_seq}


# ---- mutations of the reference's inputs: the probes must notice each ---------------------------------------------
def mutate_drop_last(p: Probe):
    """Every context one key shorter (sequences whose every row keeps at least one key)."""
    ok = [int(c) - n >= 1 for c, n in zip(p.ctx.tolist(), p.q_lens)]
    ctx = p.ctx - torch.tensor(ok, dtype=torch.int32)
    return dict(ctx=ctx), ok


def mutate_swap_v(p: Probe):
    """Per sequence, V of two neighbouring tokens of one 32-token step swapped: the first row's first needle and its
    pair partner (U: tokens 0 and 1)."""
    v = p.v.clone()
    ok = []
    for b, c in enumerate(p.ctx.tolist()):
        t = int(p.needle[int(p.qs[b]), 0]) if p.kind == "N" else 0
        u = t ^ 1
        ok.append(u < c)
        if u < c:
            bt_, bu = int(p.bt[b, t // BS]), int(p.bt[b, u // BS])
            a = v[bt_, :, :, t % BS].clone()
            v[bt_, :, :, t % BS] = v[bu, :, :, u % BS]
            v[bu, :, :, u % BS] = a
    return dict(v=v), ok


def mutate_shift_window(p: Probe):
    """Every block table shifted by one entry (entry i <- entry i + 1, the last <- the padding block)."""
    bt = torch.cat([p.bt[:, 1:], torch.full((p.B, 1), p.pad, dtype=torch.int32)], dim=1)
    return dict(bt=bt), [True] * p.B


# ---- the shapes the GPU tests launch (tests/test_decode_probes_gpu.py), also walked by the CPU tests -----------------
def _fill(fixed, n, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return fixed + torch.randint(1, hi + 1, (n - len(fixed),), generator=g).tolist()


# 1 .. 4+ steps of 32 tokens, both sides of every step edge, the 64-entry block-table window (1024 tokens) and past it
WAVE_CTX = _fill([1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 1023, 1024, 1025, 1040, 1057, 1100],
                 136, 300, 1)
# a new token at every block offset 0..15, on both sides of a 32-token step and of the 1024-token window
ROPE_CTX = _fill(list(range(1, 34)) + [48, 49, 64, 65, 1024, 1025, 1026, 1100], 130, 200, 2)
SPLIT_CTX = [1, 33, 480, 700, 2049, 4096]


def _casc_ctx(P):
    g = torch.Generator().manual_seed(P)
    out = []
    for b in range(132):
        if b % 4 == 3:  # not a member: the context ends inside (or exactly at the end of) the prefix
            out.append([BS * P, 1, BS * P - 1, 7][b // 4 % 4] if b < 32
                       else int(torch.randint(1, BS * P + 1, (1,), generator=g)))
        else:
            out.append(BS * P + ([1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65][b // 4 % 13] if b < 80
                                 else int(torch.randint(1, 121, (1,), generator=g))))
    return out


SHAPES = {
    # id: (build kwargs, fp8 allowed)
    "wave32x8": (dict(ctx=WAVE_CTX, hq=32, hkv=8, seed=11), True),
    "wave64x8": (dict(ctx=WAVE_CTX, hq=64, hkv=8, seed=12), True),
    "g1_b7_w3": (dict(ctx=[1, 16, 17, 33, 48, 40, 32], hq=4, hkv=4, width=3, seed=13), True),
    "g1_b7_w1": (dict(ctx=[1, 2, 8, 15, 16, 9, 16], hq=4, hkv=4, width=1, seed=14), True),
    "g16_b5_w1": (dict(ctx=[1, 2, 15, 16, 9], hq=16, hkv=1, width=1, seed=15), True),
    "g16_b5_w3": (dict(ctx=[48, 17, 33, 32, 1], hq=16, hkv=1, width=3, seed=16), True),
    "g16_b7_w1": (dict(ctx=[16, 1, 7, 15, 2, 16, 11], hq=16, hkv=1, width=1, seed=17), True),
    "g16_b7_w3": (dict(ctx=[1, 16, 17, 32, 33, 47, 48], hq=16, hkv=1, width=3, seed=18), True),
    "g4_b5_w1": (dict(ctx=[16, 5, 1, 15, 12], hq=8, hkv=2, width=1, seed=19), True),
    "g4_b5_w3": (dict(ctx=[5, 16, 31, 33, 48], hq=8, hkv=2, width=3, seed=20), True),
    "legacy12": (dict(ctx=WAVE_CTX[:12], hq=32, hkv=8, seed=21), True),
    "split32x8": (dict(ctx=SPLIT_CTX, hq=32, hkv=8, splits=True, seed=22), True),
    "mq4_8x2": (dict(ctx=[4096, 100, 35, 3], q_lens=[4, 1, 2, 3], hq=8, hkv=2, splits=True, seed=23), True),
    "mq4_4x1": (dict(ctx=[4096, 100, 35, 3], q_lens=[4, 1, 2, 3], hq=4, hkv=1, splits=True, seed=24), True),
    "mq2_8x2": (dict(ctx=[4096, 100, 35, 3], q_lens=[2, 1, 2, 2], hq=8, hkv=2, splits=True, seed=25), True),
    "mq2_4x1": (dict(ctx=[4096, 100, 35, 3], q_lens=[2, 1, 2, 2], hq=4, hkv=1, splits=True, seed=26), True),
    "rope32x8": (dict(ctx=ROPE_CTX, hq=32, hkv=8, rope="llama", seed=27), False),
    "rope8x2_b7": (dict(ctx=[1, 16, 17, 33, 49, 64, 1025], hq=8, hkv=2, rope="llama", seed=28), False),
    "rope16x1_b5": (dict(ctx=[1, 17, 32, 100, 33], hq=16, hkv=1, rope="llama", seed=29), False),
    "casc1": (dict(ctx=_casc_ctx(1), hq=32, hkv=8, prefix=1, rope="casc", seed=30), False),
    "casc3": (dict(ctx=_casc_ctx(3), hq=32, hkv=8, prefix=3, rope="casc", seed=31), False),
}
@functools.lru_cache(maxsize=None)
def rope_tables(which: str) -> torch.Tensor:
    """"llama": the Llama-3.1 table.  "identity" (cos 1, sin 0): the cascade's N probe — its prefix K is shared by
    sequences at different positions, which only an unrotated needle can all match (the fused-RoPE shapes cover the
    rotation)."""
    from chronos.models.llama import get_config, rope_table

    t = rope_table(get_config("llama3.1-8b"), 2048, "cpu")
    if which == "identity":
        t = torch.cat([torch.ones(2048, 64), torch.zeros(2048, 64)], dim=1)
    return t


def shape_kinds(shape: str):
    """N1: the cascade's second needle phase (the other heads' needles inside the prefix)."""
    return ("U", "N", "N1") if shape.startswith("casc") else ("U", "N")


@functools.lru_cache(maxsize=None)
def probe(shape: str, kind: str, fp8: bool = False) -> Probe:
    """The CPU probe of a GPU test shape (built once per process)."""
    kw, fp8_ok = SHAPES[shape]
    assert fp8_ok or not fp8
    kw = dict(kw)
    r = kw.pop("rope", None)
    if r == "casc":
        kw["rope"] = rope_tables("llama" if kind == "U" else "identity")
        kw["phase"] = 1 if kind == "N1" else 0
    elif r is not None:
        kw["rope"] = rope_tables(r)
    return build(kind[0], fp8=fp8, **kw)
