"""Pure-PyTorch reference implementations of every HIP kernel (the numerics oracle, and the CPU execution path).

Each function mirrors the exact contract of its kernel in csrc/kernels (same layouts, same in-place semantics) and
computes in fp32, rounding to bf16 at the same points the kernel and HF Llama do.
"""
from __future__ import annotations

import math

import torch


def embedding(ids: torch.Tensor, table: torch.Tensor, vstart: int = 0) -> torch.Tensor:
    idx = ids.long() - vstart
    ok = (idx >= 0) & (idx < table.shape[0])
    out = table[idx.clamp(0, table.shape[0] - 1)]
    return out * ok[:, None].to(out.dtype)


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * inv).to(torch.bfloat16).float().mul(w.float()).to(x.dtype)


def add_rmsnorm(x: torch.Tensor, resid: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    resid.copy_((x.float() + resid.float()).to(resid.dtype))
    return rmsnorm(resid, w, eps)


def silu_mul(gu: torch.Tensor) -> torch.Tensor:
    f = gu.shape[-1] // 2
    g, u = gu[..., :f].float(), gu[..., f:].float()
    return (torch.nn.functional.silu(g).to(torch.bfloat16).float() * u).to(gu.dtype)


FP8_MAX = 448.0


def to_fp8_bytes(x: torch.Tensor, inv_scale: float) -> torch.Tensor:
    """f32 -> OCP e4m3fn bytes with saturation (what the HIP kernels store)."""
    return (x.float() * inv_scale).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def from_fp8_bytes(b: torch.Tensor, scale: float) -> torch.Tensor:
    return b.view(torch.float8_e4m3fn).float() * scale


def quant_rows(x: torch.Tensor, resid: torch.Tensor | None = None, w: torch.Tensor | None = None, eps: float = 1e-5,
               mode: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-row dynamic e4m3 quantisation (fp8.hip quant_rows_kernel): mode 0 = x, 1 = rmsnorm(x) * w,
    2 = resid <- bf16(x + resid), rmsnorm(resid) * w, 3 = silu(gate) * up of [gate | up] rows.
    Returns (bytes [rows, d] uint8, scale [rows] f32)."""
    d = x.shape[-1]
    if mode == 3:
        y = silu_mul(x)
        d = d // 2
    elif mode == 2:
        y = add_rmsnorm(x, resid, w, eps)
    elif mode == 1:
        y = rmsnorm(x, w, eps)
    else:
        y = x
    y = y.reshape(-1, d).float()
    amax = y.abs().amax(-1)
    s = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    r = torch.where(amax > 0, FP8_MAX / amax, torch.ones_like(amax))
    q = (y * r[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, s


def qlinear(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, swiglu: bool = False) -> torch.Tensor:
    """fp32 reference of the W8A8 GEMM: (dequant(xq) @ dequant(wq).T), bf16 out; swiglu: wq = [gate; up]."""
    x = xq.view(torch.float8_e4m3fn).float()
    wf = wq.view(torch.float8_e4m3fn).float()
    acc = x @ wf.t()
    y = acc * xs.float()[:, None] * ws.float()[None, :]
    if not swiglu:
        return y.to(torch.bfloat16)
    f = y.shape[-1] // 2
    g = y[:, :f].to(torch.bfloat16).float()
    u = y[:, f:].to(torch.bfloat16).float()
    return (torch.nn.functional.silu(g).to(torch.bfloat16).float() * u).to(torch.bfloat16)


def quantize_weight(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-output-channel e4m3 weight quantisation: (bytes [N, K] uint8, scale [N] f32), w ~= bytes * scale."""
    wf = w.float()
    amax = wf.abs().amax(-1).clamp_min(1e-12)
    s = amax / FP8_MAX
    q = (wf / s[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    return q.contiguous(), s.contiguous()


MXFP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # e2m1 magnitudes by code bits 0-2


def quantize_mxfp4(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """OCP Microscaling (MX) v1.0 MXFP4 weight quantisation of w [N, K] (K % 32 == 0):
    (q uint8 [N, K / 2], e uint8 [N, K / 32]).

    * One e8m0 scale per block of 32 consecutive K elements: the shared exponent is X = floor(log2(amax)) - 2 (2 =
      e2m1's largest exponent), stored as e = X + 127 clamped to [1, 254], so that the scale 2^(e - 127) is an f32
      normal whose bit pattern is ``e << 23`` (what the decode GEMV feeds v_cvt_scalef32_pk_bf16_fp4).  An all-zero
      block takes e = 127.
    * Elements are w / 2^X, saturated to +-6, rounded to the e2m1 grid {0, .5, 1, 1.5, 2, 3, 4, 6} to nearest, ties
      to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4).
    * A code is sign in bit 3, magnitude index in bits 0-2; element 2i is the low nibble of byte i, element 2i + 1
      the high nibble.

    Every dequantised value (a 1-bit mantissa times a power of two) is exactly representable in bf16."""
    n, k = w.shape
    assert k % 32 == 0, "mxfp4: K must be a multiple of the 32-element MX block"
    wf = w.float().reshape(n, k // 32, 32)
    amax = wf.abs().amax(-1)
    _, ex = torch.frexp(amax)  # amax = m * 2^ex with m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = torch.where(amax > 0, (ex - 3 + 127).clamp(1, 254), torch.full_like(ex, 127)).to(torch.int32)
    scale = (e << 23).view(torch.float32)
    a = (wf.abs() / scale[..., None]).clamp(max=6.0)
    idx = ((a > 0.25).int() + (a >= 0.75).int() + (a > 1.25).int() + (a >= 1.75).int() + (a > 2.5).int()
           + (a >= 3.5).int() + (a > 5.0).int())
    code = (idx | (torch.signbit(wf).int() << 3)).reshape(n, k // 2, 2)
    q = (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8)
    return q.contiguous(), e.to(torch.uint8).contiguous()


def dequantize_mxfp4(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """bf16 [N, K] of MXFP4 (q [N, K / 2], e [N, K / 32]) as written by ``quantize_mxfp4``: grid[code] * 2^(e - 127),
    exact in bf16."""
    n, k = q.shape[0], q.shape[1] * 2
    qi = q.to(torch.int32)
    code = torch.stack([qi & 15, qi >> 4], -1).reshape(n, k // 32, 32)
    mag = torch.tensor(MXFP4_GRID, dtype=torch.float32, device=q.device)[(code & 7).long()]
    val = torch.where((code & 8) != 0, -mag, mag)
    scale = (e.to(torch.int32) << 23).view(torch.float32)
    return (val * scale[..., None]).reshape(n, k).to(torch.bfloat16).contiguous()


def rope_kv_write(qkv, pos, tok_seq, block_table, cos_sin, q_out, k_cache, v_cache, hq: int, hkv: int,
                  write_q: bool = True, k_scale: float = 1.0, v_scale: float = 1.0) -> None:
    T = qkv.shape[0]
    D = 128
    x = qkv.view(T, hq + 2 * hkv, D).float()
    p = pos.long()
    cos = cos_sin[p, :64].float()[:, None, :]
    sin = cos_sin[p, 64:].float()[:, None, :]
    qk = x[:, : hq + hkv]
    x1, x2 = qk[..., :64], qk[..., 64:]
    rot = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1).to(torch.bfloat16)
    if write_q:
        q_out.view(-1, hq, D)[:T].copy_(rot[:, :hq])
    bs = k_cache.shape[2]
    blk = block_table[tok_seq.long(), p // bs].long()
    off = p % bs
    v = x[:, hq + hkv:].to(torch.bfloat16)  # [T, hkv, D]
    if k_cache.dtype == torch.uint8:
        rotf = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)
        k_cache[blk, :, off, :] = to_fp8_bytes(rotf[:, hq:], 1.0 / k_scale)
        v_cache[blk, :, :, off] = to_fp8_bytes(v, 1.0 / v_scale)
    else:
        k_cache[blk, :, off, :] = rot[:, hq:]
        v_cache[blk, :, :, off] = v


def paged_attention(q, k_cache, v_cache, block_table, q_start, ctx_len, tiles=None, ntiles=0, nqt=1, nsplit=1,
                    scale: float | None = None, k_scale: float = 1.0, v_scale: float = 1.0,
                    max_q: int = 1) -> torch.Tensor:
    """Causal varlen attention over the paged cache.  q [T, Hq, 128]; seqs given by q_start/ctx_len.  Decode mode
    (tiles None): one token per sequence, or with max_q > 1 the q_start ranges (<= max_q tokens, the last at the end
    of the context) — the same causal semantics as a prefill chunk."""
    T, hq, D = q.shape
    hkv, bs = k_cache.shape[1], k_cache.shape[2]
    G = hq // hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    out = torch.zeros_like(q)
    if tiles is None and max_q == 1:  # decode: one token per sequence, seq i = token i
        qs = list(range(ntiles + 1))
    elif tiles is None:
        qs = q_start[:ntiles + 1].tolist()
    else:
        qs = q_start.tolist()
    B = len(qs) - 1
    bt = block_table.long()
    for b in range(B):
        q0, q1 = qs[b], qs[b + 1]
        ql = q1 - q0
        if ql == 0:
            continue
        ctx = int(ctx_len[b])
        nblk = (ctx + bs - 1) // bs
        blks = bt[b, :nblk]
        kb, vb = k_cache[blks], v_cache[blks]
        if k_cache.dtype == torch.uint8:  # fp8 cache: dequantise like the kernel (value * scale, then bf16)
            kb = from_fp8_bytes(kb, k_scale).to(torch.bfloat16)
            vb = from_fp8_bytes(vb, v_scale).to(torch.bfloat16)
        K = kb.permute(1, 0, 2, 3).reshape(hkv, nblk * bs, D)[:, :ctx].float()
        V = vb.permute(1, 0, 3, 2).reshape(hkv, nblk * bs, D)[:, :ctx].float()
        qq = q[q0:q1].float().view(ql, hkv, G, D)
        s = torch.einsum("qhgd,hkd->hgqk", qq, K) * scale
        qpos = torch.arange(ctx - ql, ctx, device=q.device)
        kpos = torch.arange(ctx, device=q.device)
        mask = kpos[None, :] > qpos[:, None]
        s = s.masked_fill(mask[None, None], float("-inf"))
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hgqk,hkd->qhgd", p, V)
        out[q0:q1] = o.reshape(ql, hq, D).to(q.dtype)
    return out


def ord_key(x: torch.Tensor) -> torch.Tensor:
    """Monotone 16-bit key of the bf16 rounding of x (the kernel's top-k/top-p ranking key)."""
    b = x.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b & 0x8000 != 0, (~b) & 0xFFFF, b | 0x8000)


def topkp_threshold(logits: torch.Tensor, legal: torch.Tensor, top_k: int, top_p: float) -> int:
    """Smallest key kept by top-k / top-p (llama.cpp order: raw logits), ties kept; 0 = no filtering."""
    x = logits.float()[legal]
    if x.numel() == 0:
        return 0
    keys = ord_key(x)
    thr = 0
    if top_k > 0:
        ks = torch.sort(keys, descending=True).values
        thr = max(thr, int(ks[min(top_k, ks.numel()) - 1]))
    if top_p < 1.0:
        mass = torch.exp(x - x.max())
        uk, inv = torch.unique(keys, return_inverse=True)          # ascending unique keys
        km = torch.zeros(uk.numel(), dtype=torch.float64).index_add_(0, inv, mass.double())
        cum = torch.flip(torch.cumsum(torch.flip(km, [0]), 0), [0])   # mass of keys >= uk[i]
        ok = (cum >= top_p * float(mass.sum())).nonzero()
        thr = max(thr, int(uk[int(ok.max())]) if ok.numel() else 0)
    return thr


_M32 = 0xFFFFFFFF


def _mul32(x: torch.Tensor, c: int) -> torch.Tensor:
    """x * c mod 2^32 for int64 x in [0, 2^32): two 16-bit halves of c, so no int64 product overflows."""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & _M32


def _mix32(x: torch.Tensor) -> torch.Tensor:
    """csrc/kernels/sampler.hip mix32 on int64 values masked to 32 bits."""
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def sampler_hash(seed, nout, slot, vocab: int) -> torch.Tensor:
    """The sampler kernel's 32-bit hash of tokens 0..vocab-1 (int64 tensor [..., vocab]): a pure function of (seed,
    nout, slot, token).  The three enter as ``(uint32_t)`` of an ``int32_t``, so a negative seed wraps; each may be
    an int or an integer tensor (broadcast against each other)."""
    s, n, b = (torch.as_tensor(a, dtype=torch.int64) & _M32 for a in (seed, nout, slot))
    key = _mix32(_mul32(s, 0x9E3779B9) ^ _mul32(n, 0x85EBCA6B) ^ b)
    return _mix32(key[..., None] ^ _mul32(torch.arange(vocab, dtype=torch.int64), 0xC2B2AE35))


def uniform_of_hash(hsh: torch.Tensor) -> torch.Tensor:
    """fp32 u of a 32-bit hash, as the kernel forms it: the top 23 bits plus a half, times 2^-23.  Every step is
    exact in fp32 (h + 0.5 has at most 24 significant bits), so 2^-24 <= u <= 1 - 2^-24."""
    return ((hsh >> 9).to(torch.float32) + 0.5) * (1.0 / 8388608.0)


def sampler_uniform(seed, nout, slot, vocab: int) -> torch.Tensor:
    """The uniform the sampler kernel draws for tokens 0..vocab-1 at (seed, nout, slot): fp32, bit for bit."""
    return uniform_of_hash(sampler_hash(seed, nout, slot, vocab))


def constrained_sample(logits, row_of_slot, next_tab, dist, done_state: int, state, remaining, temperature, seed,
                       ids, pos, ctx, nout, out_tokens, topk=None, topp=None, jump=None) -> None:
    """Greedy / Gumbel-max sampling restricted by the token DFA; advances the slot state in place (host loop).
    A row entering a state flagged in ``jump`` is parked as ``-2 - state``.  Sampled rows draw the kernel's own
    counter-hash stream (``sampler_uniform``) and score in fp64, so both backends pick the same token for the same
    (seed, step, slot) unless the two best scores lie within the kernel's fp32 rounding of each other."""
    n = state.numel()
    V = next_tab.shape[1]
    for slot in range(n):
        s = int(state[slot])
        if s < 0 or s == done_state:
            continue
        row = int(row_of_slot[slot]) if row_of_slot is not None else slot
        if row < 0:
            continue
        nx = next_tab[s].long()
        budget = int(remaining[slot]) - 1
        legal = (nx >= 0)
        legal &= dist[nx.clamp(min=0)].long() <= budget
        if not bool(legal.any()):
            state[slot] = done_state
            continue
        sc = logits[row, :V].float()
        t = float(temperature[slot]) if temperature is not None else 0.0
        tk = int(topk[slot]) if topk is not None else 0
        tp = float(topp[slot]) if topp is not None else 1.0
        if t > 0 and (tk > 0 or tp < 1.0):
            thr = topkp_threshold(sc, legal, tk, tp)
            legal = legal & (ord_key(sc) >= thr)
        if t > 0:
            u = sampler_uniform(int(seed[slot]) if seed is not None else 0, int(nout[slot]), slot, V).to(sc.device)
            sc = sc.double() / t - torch.log(-torch.log(u.double()))
        sc = sc.masked_fill(~legal, float("-inf"))
        tok = int(torch.argmax(sc))
        ns = int(nx[tok])
        k = int(nout[slot])
        if k < out_tokens.shape[1]:
            out_tokens[slot, k] = tok
        nout[slot] = k + 1
        remaining[slot] = budget
        park = jump is not None and ns != done_state and 0 < int(jump[ns]) <= budget
        state[slot] = -2 - ns if park else ns
        if ns != done_state:
            ids[slot] = tok
            pos[slot] += 1
            ctx[slot] += 1


def token_logprobs(logits, row_of_slot, next_tab, dist, done_state: int, state, remaining, nout, lp_want, lp_mark,
                   lp_lse, lp_top_ids, lp_top_val) -> None:
    """fp32 reference of csrc/kernels/logprobs.hip token_logprobs_kernel (host loop over the slots)."""
    V, K = next_tab.shape[1], lp_top_ids.shape[1]
    for slot in range(state.numel()):
        s = int(state[slot])
        row = -1 if (s < 0 or s == done_state) else (int(row_of_slot[slot]) if row_of_slot is not None else slot)
        if row < 0 or int(lp_want[slot]) < 0:
            lp_mark[slot] = -1
            continue
        nx = next_tab[s].long()
        legal = (nx >= 0) & (dist[nx.clamp(min=0)].long() <= int(remaining[slot]) - 1)
        idx = legal.nonzero().flatten()
        if idx.numel() == 0:
            lp_mark[slot] = -1
            continue
        x = logits[row, :V].float()[idx]
        mx = float(x.max())
        mx = 0.0 if mx == float("-inf") else mx
        lp_lse[slot] = mx + float(torch.log(torch.exp(x - mx).sum()))
        order = torch.sort(-(x + 0.0), stable=True).indices[:K]  # idx ascends, so equal logits keep id order
        k = order.numel()
        lp_top_ids[slot, :k] = idx[order].to(lp_top_ids.dtype)
        lp_top_val[slot, :k] = x[order]
        lp_top_ids[slot, k:] = -1
        lp_top_val[slot, k:] = float("-inf")
        lp_mark[slot] = int(nout[slot])


def token_logprobs_commit(logits, row_of_slot, nout, out_tokens, lp_want, lp_mark, lp_lse, lp_top_ids, lp_top_val,
                          out_lp, out_lp_ids) -> None:
    """fp32 reference of token_logprobs_commit_kernel."""
    max_out = out_tokens.shape[1]
    for slot in range(nout.numel()):
        i = int(lp_mark[slot])
        if i < 0 or i >= max_out or int(lp_want[slot]) < 0 or int(nout[slot]) != i + 1:
            continue
        row = int(row_of_slot[slot]) if row_of_slot is not None else slot
        if row < 0:
            continue
        lse = lp_lse[slot]
        out_lp[slot, i, 0] = logits[row, int(out_tokens[slot, i])].float() - lse
        out_lp[slot, i, 1:] = lp_top_val[slot] - lse
        out_lp_ids[slot, i] = lp_top_ids[slot]


def apply_penalties(logits, row_of_slot, done_state: int, state, nout, out_tokens, pen_par, pen_last, pen_tail,
                    pen_tlen) -> None:
    """fp32 reference of csrc/kernels/penalties.hip (host loop over the slots, torch.unique for the counts); the
    penalised values are rounded to the logits dtype at the end, as the kernel's store does."""
    W, max_out, width = pen_tail.shape[1], out_tokens.shape[1], logits.shape[1]
    for slot in range(state.numel()):
        s = int(state[slot])
        if s < 0 or s == done_state:
            continue
        row = int(row_of_slot[slot]) if row_of_slot is not None else slot
        L = min(int(pen_last[slot]), W)
        rp, fq, pr = (pen_par[slot, i] for i in range(3))  # f32 scalars: the arithmetic below stays in fp32
        if row < 0 or L <= 0 or (float(rp) == 1.0 and float(fq) == 0.0 and float(pr) == 0.0):
            continue
        tl = min(max(int(pen_tlen[slot]), 0), W)
        no = min(max(int(nout[slot]), 0), max_out)
        hist = torch.cat([pen_tail[slot, :tl].long(), out_tokens[slot, :no].long()])[-L:]
        hist = hist[(hist >= 0) & (hist < width)]
        if hist.numel() == 0:
            continue
        ids, cnt = torch.unique(hist, return_counts=True)
        x = logits[row, ids].float()
        x = torch.where(x <= 0, x * rp, x / rp)
        x = x - (cnt.float() * fq + pr)
        logits[row, ids] = x.to(logits.dtype)


def truncate_survivors(x: torch.Tensor, legal: torch.Tensor, minp_ln: float, typical: float,
                       dtype=torch.float32) -> torch.Tensor:
    """Survivor mask of one logits row under typical_p then min_p (llama.cpp's semantics on raw logits, over the
    legal tokens only; csrc/kernels/truncate.hip).  ``x`` [V] logits, ``legal`` [V] bool, ``minp_ln`` = ln(min_p)
    (-inf = off), ``typical`` = typical_p (>= 1 = off).  Returns a bool [V] mask, a subset of ``legal``; with at most
    one legal token, or no legal logit above -inf, it is ``legal`` itself.  ``dtype``: the arithmetic's precision
    (float64 gives the tests their yardstick); the min_p comparison is always the fp32 ``x >= m' + ln p``."""
    keep = legal.clone()
    idx = legal.nonzero().flatten()
    if idx.numel() < 2:
        return keep
    xf = x.float()[idx]
    if float(xf.max()) == float("-inf"):
        return keep
    alive = torch.ones_like(xf, dtype=torch.bool)
    if typical < 1.0:
        xl = xf.to(dtype)
        dx = xl - xl.max()
        e = torch.exp(dx)
        logp = dx - torch.log(e.sum())
        p = e / e.sum()
        H = -(torch.where(p > 0, p * logp, torch.zeros_like(p))).sum()
        d = (-logp - H).abs()
        order = torch.sort(d, stable=True).indices
        cum = torch.cumsum(p[order], 0)
        over = (cum > typical).nonzero().flatten()
        dstar = d[order[int(over[0])]] if over.numel() else d[order[-1]]
        alive = d <= dstar
    if minp_ln > float("-inf"):
        m2 = xf[alive].max()
        alive = alive & (xf >= m2 + torch.tensor(minp_ln, dtype=torch.float32))
    keep[idx] = alive
    return keep


def truncate_logits(logits, row_of_slot, next_tab, dist, done_state: int, state, remaining, temperature, minp_ln,
                    typical) -> None:
    """fp32 reference of csrc/kernels/truncate.hip (host loop over the slots): -inf, in place, into the legal tokens
    of each live sampling slot that typical_p and then min_p remove."""
    V = next_tab.shape[1]
    for slot in range(state.numel()):
        s = int(state[slot])
        if s < 0 or s == done_state:
            continue
        row = int(row_of_slot[slot]) if row_of_slot is not None else slot
        lnp, tp = float(minp_ln[slot]), float(typical[slot])
        if row < 0 or not float(temperature[slot]) > 0.0 or (lnp == float("-inf") and not tp < 1.0):
            continue
        nx = next_tab[s].long()
        legal = (nx >= 0) & (dist[nx.clamp(min=0)].long() <= int(remaining[slot]) - 1)
        keep = truncate_survivors(logits[row, :V], legal, lnp, tp)
        kill = (legal & ~keep).nonzero().flatten()
        if kill.numel():
            logits[row, kill] = float("-inf")


_INV_LN2 = 1.4426950408889634


def mirostat_row(x: torch.Tensor, legal: torch.Tensor, temperature: float, mu: float, dtype=torch.float32):
    """One row of Mirostat 2.0's truncation (csrc/kernels/mirostat.hip, steps 1 to 3): over the ``legal`` tokens of
    logits row ``x`` [V], with ``m = max x`` and ``Z = sum exp((x - m) / T)``, the surprise in bits is
    ``S = ((m - x) / T + ln Z) / ln 2``; a token survives iff ``S <= mu`` or ``x == m``.  Returns ``(keep, m, lnz)``:
    the bool [V] survivor mask (a subset of ``legal``), the maximum and ``ln Z'`` of the survivors as 0-d tensors of
    ``dtype`` — or ``None`` for a forced step (fewer than two legal tokens, or no legal logit above -inf).  ``dtype``:
    the arithmetic's precision (float64 gives the tests their yardstick)."""
    idx = legal.nonzero().flatten()
    if idx.numel() < 2:
        return None
    xl = x.float()[idx].to(dtype)
    m = xl.max()
    if float(m) == float("-inf"):
        return None
    T = torch.tensor(temperature, dtype=torch.float32).to(dtype)
    e = torch.exp((xl - m) / T)
    s = ((m - xl) / T + torch.log(e.sum())) * torch.tensor(_INV_LN2, dtype=dtype)
    alive = (xl == m) | (s <= torch.tensor(mu, dtype=torch.float32).to(dtype))
    keep = torch.zeros_like(legal)
    keep[idx] = alive
    return keep, m, torch.log(e[alive].sum())


def mirostat_truncate(logits, row_of_slot, next_tab, dist, done_state: int, state, remaining, nout, temperature, mi_on,
                      mi_mu, mi_m, mi_lnz, mi_mark) -> None:
    """fp32 reference of mirostat_truncate_kernel (host loop over the slots): -inf, in place, into the legal tokens of
    each live sampling slot with mirostat on whose surprise exceeds the slot's mu; ``mi_m`` / ``mi_lnz`` / ``mi_mark =
    nout`` for the update.  Every slot it does not truncate — skipped, greedy, off, forced — gets ``mi_mark = -1``."""
    V = next_tab.shape[1]
    for slot in range(state.numel()):
        mi_mark[slot] = -1
        s = int(state[slot])
        row = int(row_of_slot[slot]) if row_of_slot is not None else slot
        T = float(temperature[slot])
        if not int(mi_on[slot]) or s < 0 or s == done_state or row < 0 or not T > 0.0:
            continue
        nx = next_tab[s].long()
        legal = (nx >= 0) & (dist[nx.clamp(min=0)].long() <= int(remaining[slot]) - 1)
        res = mirostat_row(logits[row, :V], legal, T, float(mi_mu[slot]))
        if res is None:
            continue
        keep, m, lnz = res
        kill = (legal & ~keep & (logits[row, :V].float() > float("-inf"))).nonzero().flatten()
        if kill.numel():
            logits[row, kill] = float("-inf")
        mi_m[slot] = m
        mi_lnz[slot] = lnz
        mi_mark[slot] = int(nout[slot])


def mirostat_update(logits, row_of_slot, nout, out_tokens, temperature, mi_on, mi_mu, mi_tau, mi_eta, mi_m, mi_lnz,
                    mi_mark) -> None:
    """fp32 reference of mirostat_update_kernel: where the sampler emitted output index ``i = mi_mark[slot]`` (``nout
    == i + 1``) with token ``t``, ``S_obs = ((m - x_t) / T + ln Z') / ln 2`` and ``mu <- mu - eta * (S_obs - tau)``."""
    max_out = out_tokens.shape[1]
    for slot in range(nout.numel()):
        i = int(mi_mark[slot])
        if i < 0 or i >= max_out or not int(mi_on[slot]) or int(nout[slot]) != i + 1:
            continue
        row = int(row_of_slot[slot]) if row_of_slot is not None else slot
        T = temperature[slot].float()
        tok = int(out_tokens[slot, i])
        if row < 0 or not float(T) > 0.0 or not 0 <= tok < logits.shape[1]:
            continue
        sobs = ((mi_m[slot] - logits[row, tok].float()) / T + mi_lnz[slot]) * torch.tensor(_INV_LN2)
        if not bool(torch.isfinite(sobs)):
            continue
        mi_mu[slot] = mi_mu[slot] - mi_eta[slot] * (sobs - mi_tau[slot])


POOL_HIDDEN = (256, 1024, 4096, 8192)  # the hidden sizes csrc/kernels/pool.hip is compiled for


def pool_accum(s: torch.Tensor, eps: float, q_rows: torch.Tensor, sel: torch.Tensor, acc: torch.Tensor) -> None:
    """acc[sel[b]] += sum over rows r in [q_rows[b, 0], q_rows[b, 1]) of s[r] * rsqrt(mean(s[r]^2) + eps), accumulated in
    fp64 and added to the fp32 accumulator once per sequence (csrc/kernels/pool.hip).  ``sel[b] < 0`` (or past the
    accumulator) skips the sequence, a range is clipped to the rows of ``s``, rows outside every range are never read."""
    T, S = s.shape[0], acc.shape[0]
    for b, row in enumerate(sel.tolist()):
        if not 0 <= row < S:
            continue
        lo, hi = max(int(q_rows[b, 0]), 0), min(int(q_rows[b, 1]), T)
        if hi <= lo:
            continue
        x = s[lo:hi].double()
        inv = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
        acc[row] = (acc[row].double() + (x * inv).sum(0)).to(acc.dtype)


def pool_finish(acc: torch.Tensor, rows: torch.Tensor, g: torch.Tensor, out: torch.Tensor) -> None:
    """out[i] = v / ||v||_2 with v = g * acc[rows[i]] (fp64; zeros when the norm is 0), then acc[rows[i]] <- 0.  A row
    outside the accumulator gives zeros."""
    S = acc.shape[0]
    for i, row in enumerate(rows.tolist()):
        if not 0 <= row < S:
            out[i] = 0
            continue
        v = acc[row].double() * g.double()
        n = v.pow(2).sum().sqrt()
        out[i] = (v / n).to(out.dtype) if n > 0 else 0
        acc[row] = 0
