"""Shared cases of the MXFP4 tests (test_mxfp4.py on the CPU, test_mxfp4_gpu.py on the GPU): hand-worked MX blocks,
the code table, the probe columns and small builders.  No test lives here."""
import torch

GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # e2m1 magnitude by code bits 0-2; bit 3 is the sign

# (value, expected code) inside a block whose amax is 5.0 (floor(log2) = 2 -> X = 0, e = 127, scale 1): the ties go to
# the even code, with both signs.  -0.25 rounds to -0: sign bit set, magnitude 0.
TIES = [(0.25, 0), (-0.25, 8), (0.75, 2), (-0.75, 10), (1.25, 2), (-1.25, 10), (1.75, 4), (-1.75, 12), (2.5, 4),
        (-2.5, 12), (3.5, 6), (-3.5, 14), (5.0, 6), (-5.0, 14), (0.5, 1), (1.0, 2), (1.5, 3), (2.0, 4), (3.0, 5),
        (4.0, 6), (-3.0, 13), (0.0, 0)]


def block(vals) -> torch.Tensor:
    """One row of one MX block (32 elements, zero padded) as bf16 [1, 32]."""
    v = torch.zeros(32)
    v[:len(vals)] = torch.tensor(list(vals), dtype=torch.float32)
    return v.to(torch.bfloat16).view(1, 32)


def codes_of(q: torch.Tensor) -> torch.Tensor:
    """[N, K] codes from packed bytes [N, K / 2]: element 2i = low nibble of byte i, element 2i + 1 = high nibble."""
    qi = q.to(torch.int32)
    return torch.stack([qi & 15, qi >> 4], -1).reshape(q.shape[0], -1)


def pack(codes: torch.Tensor) -> torch.Tensor:
    c = codes.to(torch.int32).reshape(codes.shape[0], -1, 2)
    return (c[..., 0] | (c[..., 1] << 4)).to(torch.uint8).contiguous()


def table_value(code: int, e: int) -> float:
    """grid[code] * 2^(e - 127) in exact Python arithmetic."""
    mag = GRID[code & 7] * 2.0 ** (e - 127)
    return -mag if code & 8 else mag


def probe_columns(k: int, seed: int) -> list[int]:
    """All of [0, 64), all of [K - 64, K) and 64 seeded others."""
    g = torch.Generator().manual_seed(seed)
    mid = (64 + torch.randperm(k - 128, generator=g)[:64]).tolist() if k > 192 else []
    return sorted(set(range(64)) | set(range(k - 64, k)) | set(mid))


def spread_weight(n: int, k: int, seed: int, device="cpu") -> torch.Tensor:
    """Random bf16 [N, K] whose MX blocks' magnitudes spread over 2^-16 .. 2^9, so the shared exponents of their
    quantisation (126 + the block's exponent, the amax of 32 Gaussians lying in [2, 4)) cover about [110, 135]."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k // 32, 32, generator=g)
    ex = torch.randint(-16, 10, (n, k // 32, 1), generator=g).float()
    return (w * torch.exp2(ex)).reshape(n, k).to(torch.bfloat16).to(device)
