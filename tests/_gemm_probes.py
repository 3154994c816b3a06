"""Exact integer probes for the projection GEMMs (csrc/kernels/gemm_pp.hip, gemm_lg.hip, gemm_skinny.hip, gemv.hip,
gemm.hip and gemm_lg.hip's fp8 configs), shared by tests/test_gemm_probes.py (CPU: builder proofs and mutation checks)
and tests/test_gemm_probes_gpu.py (the HIP kernels).  Torch only, device-agnostic, vectorised.

Why.  The older GEMM tests draw random operands and allow ``1e-2..3e-2 * max|ref|``: at K = 4096 one product term is
0.03-0.07 against an allowance of about 0.065, so a lane that drops or doubles one k element, loses a 16-B piece, pairs
an x column with the neighbouring w column or loses one split-K slab row passes.  Here every operand is a small integer
and every partial sum is an integer far below 2^24, so the result does not depend on accumulation order, split-K or tile
shape, and the comparison is ``torch.equal``.

x     [M, K] bf16, integers uniform in {-2, .., 2}.
w     [N, K] bf16 in {-1, 0, +1}: every aligned group of G consecutive rows against every aligned block of G consecutive
      k holds a random permutation matrix with random signs — every k is touched exactly once per G-row group, every row
      has exactly K / G non-zeros.  G = max(16, K / 64) (``group``); a last group with fewer than G rows keeps only its
      own rows.  Hence |x w^T| <= 2 K / G <= 128, an integer: exact in fp32 partial sums in any order and exact in
      bf16.  16 is the smallest MFMA row tile, so every 16-row fragment of a K <= 1024 probe sees every k.
resid [M, N] bf16, integers in [-64, 64]: s = bf16(bf16(x w^T) + r) is an integer with |s| <= 192, exact.  Every RMSNorm
      partial is a sum of at most 256 squares <= 192^2 < 2^24: exact in fp32 in any order; the test sums the partial
      columns in fp64 and compares with the exact sum of s^2 by equality.  ``frac=True`` is the non-integer variant:
      r = j / 64 with |j| <= 127 (exact in bf16), so y + r is exact in fp32 but needs 14 bits wherever |y| >= 2 and the
      bf16 store must round it.  s is still one correct rounding of an exact sum (``torch.equal``), but partials taken
      from the sum before the store differ from the partials of what was stored by about 2^-8 of each term; the
      partials themselves are then fp32 sums of n <= 256 non-negative terms, within (n + 1) 2^-24 of the exact sum in
      any order (``part_bound``) — some thirty times less than the difference.
SwiGLU (w = [gate; up]): the gate half uses G = K / 16, so gate rows have 16 non-zeros and |g| <= 32: silu(g) stays a
      normal float and an off-by-one in g moves the result by a large factor (silu(g - 1) / silu(g) is about e for
      g << 0, and (g + 1) / g above).  Each integer pair (g, u) is exact; the expectation is silu(g) u in fp64.
part_in (folded RMSNorm prologue, independent of x — the kernels read it, they do not recompute it): row sums such that
      inv = rsqrt(sum / K + eps) is within 1e-6 of one of {2, 1, 1/2, 1/4}, the class walking over the rows by seeded
      non-zero steps so neighbouring rows always differ by >= 2x, and the mass split evenly over 1-4 randomly chosen
      columns of the P, one of which is column (P - 1 - row) % P (row 0 holds mass in the last column: a kernel that sums
      too few columns gets that row's inv wrong by >= 15 %).  The expectation uses the fp64 inv of the fp32 values passed.

Bounds (derived, not measured).  Plain, residual and the residual's partials: equality.  SwiGLU and the norm prologue:
|y - e| <= 2^-7 |e| + 1e-30.  All kernels round the scaled gate and up values to bf16 before silu (the unfused chain
rounds the GEMM output there): on these probes that rounding is exact or restores the exact value — g and u are
integers <= 256 in magnitude, inv is a power of two up to 1e-6, and bf16(2^j v (1 + 1e-6)) = 2^j v — so what is left
is the fp32 silu (``__expf``: the exponent's product with log2 e carries |g| 2^-24 relative, below 1e-5 at |g| <= 64),
its bf16 rounding (2^-9), the bf16 store (2^-9) and the expectation's own inv error times silu's sensitivity
(|inv g| + 2) 1e-6 < 1e-4: together below 2^-8 + 2e-4 < 2^-7.

Poison.  ``carve`` puts every operand as a contiguous view, at a multiple of 256 B, inside a larger buffer filled with
NaN (fp8 bytes: 0x7F, e4m3fn's NaN): a read outside an operand that reaches a stored output shows up as NaN.
"""
from __future__ import annotations

import torch

BF16 = torch.bfloat16
EPS = 1e-5
REL = 2.0 ** -7  # SwiGLU / norm-prologue bound, relative to the fp64 expectation
ABS = 1e-30
INV_CLASSES = (2.0, 1.0, 0.5, 0.25)
PAD_BYTES = 4096  # poison on each side of an operand (a multiple of 256)


def group(k: int) -> int:
    return max(16, k // 64)


def _gen(seed: int, device) -> torch.Generator:
    return torch.Generator(device=device).manual_seed(int(seed))


def carve(t: torch.Tensor) -> torch.Tensor:
    """A contiguous copy of ``t`` inside a NaN-filled buffer, PAD_BYTES of poison on each side."""
    pad = PAD_BYTES // t.element_size()
    if t.dtype == torch.uint8:
        buf = torch.full((t.numel() + 2 * pad,), 0x7F, dtype=torch.uint8, device=t.device)
    else:
        buf = torch.full((t.numel() + 2 * pad,), float("nan"), dtype=t.dtype, device=t.device)
    v = buf[pad:pad + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 256 == buf.data_ptr() % 256
    return v


def guard_ok(v: torch.Tensor) -> bool:
    """True while the poison around a ``carve`` view is untouched (for outputs a kernel writes in place)."""
    pad = PAD_BYTES // v.element_size()
    base = v.new_empty(0).set_(v.untyped_storage(), 0, (v.numel() + 2 * pad,))
    lo, hi = base[:pad], base[pad + v.numel():]
    if v.dtype == torch.uint8:
        return bool((lo == 0x7F).all() and (hi == 0x7F).all())
    return bool(lo.isnan().all() and hi.isnan().all())


def make_x(m: int, k: int, seed: int, device="cpu") -> torch.Tensor:
    return torch.randint(-2, 3, (m, k), generator=_gen(seed, device), device=device).to(BF16)


def make_w(n: int, k: int, seed: int, device="cpu", g: int | None = None) -> torch.Tensor:
    g = g or group(k)
    assert k % g == 0, (k, g)
    rg, kb = -(-n // g), k // g
    gen = _gen(seed, device)
    perm = torch.rand(rg, kb, g, generator=gen, device=device).argsort(-1)  # row i of block (rg, kb) -> its column
    sign = torch.randint(0, 2, (rg, kb, g), generator=gen, device=device) * 2 - 1
    w = torch.zeros(rg, g, kb, g, device=device)
    w.scatter_(3, perm.permute(0, 2, 1).unsqueeze(-1), sign.permute(0, 2, 1).unsqueeze(-1).float())
    return w.view(rg * g, k)[:n].to(BF16).contiguous()


def make_w_swiglu(f: int, k: int, seed: int, device="cpu") -> torch.Tensor:
    """[2F, K] = [gate; up]: gate rows with 16 non-zeros (G = K / 16), up rows with the default G."""
    assert k % 16 == 0
    return torch.cat([make_w(f, k, seed, device, k // 16), make_w(f, k, seed + 1, device)], 0).contiguous()


def make_resid(m: int, n: int, seed: int, device="cpu", frac: bool = False) -> torch.Tensor:
    if frac:
        return (torch.randint(-127, 128, (m, n), generator=_gen(seed, device), device=device).float() / 64).to(BF16)
    return torch.randint(-64, 65, (m, n), generator=_gen(seed, device), device=device).to(BF16)


def inv_classes(m: int, seed: int, device="cpu") -> torch.Tensor:
    """Class index (into INV_CLASSES) per row: a seeded walk with non-zero steps, so neighbours always differ."""
    gen = _gen(seed, device)
    steps = torch.randint(1, 4, (m,), generator=gen, device=device)
    return steps.cumsum(0) % 4


def make_parts(m: int, k: int, p: int, seed: int, device="cpu", eps: float = EPS) -> torch.Tensor:
    """[M, P] f32 producer partials: see the module docstring."""
    cls = inv_classes(m, seed, device)
    inv = torch.tensor(INV_CLASSES, dtype=torch.float64, device=device)[cls]
    total = k * (inv ** -2 - eps)
    gen = _gen(seed + 1, device)
    ncol = torch.randint(1, min(4, p) + 1, (m,), generator=gen, device=device)
    score = torch.rand(m, p, generator=gen, device=device)
    forced = (p - 1 - torch.arange(m, device=device)) % p
    score.scatter_(1, forced[:, None], -1.0)
    rank = score.argsort(1).argsort(1)
    mask = rank < ncol[:, None]
    return ((total / ncol)[:, None] * mask).float().contiguous()


def inv_of(part: torch.Tensor, k: int, eps: float = EPS) -> torch.Tensor:
    """fp64 [M, 1] rsqrt(sum / K + eps) of the fp32 partials actually passed."""
    return torch.rsqrt(part.double().sum(1, keepdim=True) / k + eps)


def expect_plain(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """fp64 x w^T from the integer operands (every product and sum an integer below 2^53: exact)."""
    return x.double() @ w.double().t()


def expect_swiglu(x: torch.Tensor, w: torch.Tensor, inv: torch.Tensor | None = None) -> torch.Tensor:
    h = expect_plain(x, w)
    if inv is not None:
        h = h * inv
    f = w.shape[0] // 2
    g, u = h[:, :f], h[:, f:]
    return g / (1.0 + torch.exp(-g)) * u


def expect_resid(x: torch.Tensor, w: torch.Tensor, r: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(s as bf16, exact fp64 row sums of s^2) of s = bf16(bf16(x w^T) + r).  y is an integer <= 128 and r a multiple
    of 1/64 below 2, so y + r is exact in fp64 (and in fp32) and the one rounding is the final bf16 store."""
    y = expect_plain(x, w)
    s = (y + r.double()).to(BF16)
    return s, (s.double() ** 2).sum(1)


def part_bound(exact: torch.Tensor, cols: int) -> torch.Tensor:
    """Allowance for an fp32 sum of ``cols`` non-negative squares (the ``frac`` residual's partials)."""
    return (cols + 1) * 2.0 ** -24 * exact


def close(y: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """Elementwise: inside the SwiGLU / norm-prologue bound (NaN is outside)."""
    return (y.double() - e).abs() <= REL * e.abs() + ABS


# ---- fp8 (e4m3fn bytes) ------------------------------------------------------------------------------------------
def to_e4m3(t: torch.Tensor) -> torch.Tensor:
    """uint8 e4m3fn bytes of a tensor of small integers (|v| <= 2: exact)."""
    q = t.float().to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), t.float())
    return q.view(torch.uint8)


def pow2_scales(n: int, device="cpu") -> torch.Tensor:
    """f32 [n]: 2^((i mod 3) - 1)."""
    return torch.pow(2.0, (torch.arange(n, device=device) % 3 - 1).float())
