"""Exact integer probes for the mid-M W4A16 GEMM (csrc/kernels/gemm_w4m.hip), shared by tests/test_mxfp4_mid.py (CPU:
builder proofs and mutation checks) and tests/test_mxfp4_mid_gpu.py (the kernel).  Everything but the weight encoding
comes from tests/_gemm_probes.py (``make_x``, ``make_w``, ``make_w_swiglu``, ``make_resid``, ``make_parts``,
``expect_*``, ``carve``, ``guard_ok``, ``close``) and tests/_mxfp4_cases.py (``pack``); no test lives here.

``encode_pm1`` turns the probes' {-1, 0, +1} weight matrix into MXFP4 bytes whose dequantisation is that matrix bit for
bit, while making the block scale matter: per MX block (32 consecutive k of one row) the ±1 entries use one of four
exact encodings

    class   code (magnitude bits)   value   e8m0      value * 2^(e - 127)
      0             1                0.5    128              1
      1             2                1      127              1
      2             4                2      126              1
      3             6                4      125              1

with class = (row + walk[block]) % 4, ``walk`` a seeded cumulative sum of steps in {1, 2, 3}: neighbouring rows and
neighbouring blocks never share a scale, so a kernel that pairs a block's codes with a neighbour's scale byte — the next
block of the row, or the same block of the next row — is off by a factor 2, 4 or 8 wherever the block has a non-zero.
``make_w(..., g=32)`` (K <= 4096) puts exactly one non-zero into every block of every row, so every such exchange shows
in every output that touches the block with a non-zero x; |x w^T| <= 2 K / 32 <= 256 stays exact in bf16.
"""
from __future__ import annotations

import torch

import _gemm_probes as P
from _mxfp4_cases import pack

CLASS_CODE = (1, 2, 4, 6)        # e2m1 magnitude codes of 0.5, 1, 2, 4
CLASS_E = (128, 127, 126, 125)   # the e8m0 byte that scales each back to 1


def probe_g(k: int):
    """``make_w``'s group size for the W4 probes: one non-zero per row and MX block up to K = 4096, the default above."""
    return 32 if k <= 4096 else None


def block_classes(n: int, nb: int, seed: int, device="cpu") -> torch.Tensor:
    """[n, nb] class index of every (row, MX block)."""
    gen = torch.Generator(device=device).manual_seed(int(seed))
    walk = torch.randint(1, 4, (nb,), generator=gen, device=device).cumsum(0)
    return (torch.arange(n, device=device)[:, None] + walk[None, :]) % 4


def encode_pm1(w: torch.Tensor, seed: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(q uint8 [N, K / 2], e uint8 [N, K / 32]) of a bf16 matrix with entries in {-1, 0, +1}."""
    n, k = w.shape
    assert k % 32 == 0
    wf = w.float()
    assert bool(((wf == 0) | (wf.abs() == 1)).all())
    cls = block_classes(n, k // 32, seed, w.device)
    code = torch.tensor(CLASS_CODE, device=w.device)[cls]                      # [n, nb]
    e = torch.tensor(CLASS_E, dtype=torch.uint8, device=w.device)[cls].contiguous()
    mag = code[:, :, None].expand(n, k // 32, 32).reshape(n, k)
    codes = torch.where(wf != 0, mag + 8 * (wf < 0), torch.zeros_like(mag))
    return pack(codes), e


def make_w4(n: int, k: int, seed: int, device="cpu"):
    """(w bf16 [N, K] in {-1, 0, +1}, q, e) — plain / residual weights."""
    w = P.make_w(n, k, seed, device, probe_g(k))
    q, e = encode_pm1(w, seed + 5)
    return w, q, e


def make_w4_swiglu(f: int, k: int, seed: int, device="cpu"):
    """(w = [gate; up] bf16 [2F, K], q, e): ``_gemm_probes.make_w_swiglu`` (gate rows with 16 non-zeros)."""
    w = P.make_w_swiglu(f, k, seed, device)
    q, e = encode_pm1(w, seed + 5)
    return w, q, e
