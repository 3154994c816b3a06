"""Exact per-key probes (tests/_prefill_probes.py) through every prefill-attention instantiation that
``launch_attn_prefill`` (csrc/kernels/attention_prefill.hip) and, for nqt = 2, ``launch_paged_attn``
(csrc/kernels/attention.hip) can dispatch.

U (uniform: K = 0, one-hot V) says which keys were attended, C (comb: Hadamard-class keys, position-coded V) says
which V went with which K; poison around every context says what was read that should not have been.  The bounds are
derived in tests/_prefill_probes.py (2^-7 relative, the decode probes' bounds: the bf16 store of the output rounds by
2^-9) — one wrong key is at least twice outside them in every row it touches.  A failure prints the probe's signature:
the dims off and by how many counts (U), or which class member is missing, extra or came back with another key's V (C).

Instantiation -> how ``VARIANTS`` selects it (knobs are set for the call and erased again):

  launch_attn_prefill (nqt = 8, a tile list)
    attn_prefill_kernel<F, 1 | 2>          ``variant`` = prefill_variant 0 | 1: neither ``variant == 2 || variant == 5``
                                           nor (fp8) ``f8`` (it needs variant == 2); ``sub = variant == 1 ? 2 : 1``
    attn_prefill2_kernel<bf16, LEAN, WPG>  the defaults: ``variant == 2 && block_size == 16``, knob prefill_wpg = 1
    attn_prefill2_kernel<bf16, LEAN>       prefill_wpg = 0
    attn_prefill2_kernel<fp8, LEAN>        prefill_fp8_mfma = 0 -> ``f8`` = 0; and, at the default knobs, a kv head
                                           count that is no power of two (hq / hkv = 12 / 3: ``(hkv & (hkv - 1)) == 0``
                                           fails -> ``f8`` = 0)
    attn_prefill2_kernel<F, non-LEAN>      page size 32 (``block_size == 16`` fails: the ``else`` of AP2_LAUNCH; fp8
                                           too, ``f8`` needs block_size 16), and prefill_variant = 5
    attn_prefill8_kernel<PV8, FOLD, MSUM, PIPE, WPG>   fp8, page 16, power-of-two hkv, prefill_fp8_mfma = 1 .. 8:
                                           1 <1,0,0,0,1>  2 <0,1,0>  3 <1,1,1>  4 <0,0,0>  5 <1,0,1>  6 <1,0,0,1>
                                           7 <1,0,0>  8 <1,0,1,0,1>
  launch_paged_attn (nqt = 2: PA_LAUNCH(2, fp8))
    paged_attn_kernel<2, F>                nsplit 1; nsplit 3 (``nsplit <= knob("inkernel_combine_max_split", 4)``:
                                           the last split's in-launch ticket combine); nsplit 8 (``cnt == nullptr``:
                                           paged_attn_combine_kernel<2>)
"""
import contextlib
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prefill_probes as pp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
KNOBS = ("prefill_variant", "prefill_fp8_mfma", "prefill_wpg", "inkernel_combine_max_split")

# one launch per shape: the smallest shapes at which a variant can still go wrong (tests/_prefill_probes.py SHAPES)
PAGE16 = ("ragged32x8", "ragged64x8", "ragged16x1", "ragged4x4", "g1_two_tiles", "long_u")
PAGE32 = ("ragged32x8_p32", "ragged16x1_p32", "g1_two_tiles_p32")
SPLIT = ("ragged32x8_split", "ragged4x4_split", "ragged16x1_split", "ragged32x8_p32_split", "ragged64x8",
         "g1_two_tiles", "long_u")


def _v(name, fp8, shapes, nqt=8, nsplit=1, **knobs):
    return pytest.param(dict(fp8=fp8, shapes=shapes, nqt=nqt, nsplit=nsplit, knobs=knobs), id=name)


VARIANTS = (
    # attn_prefill_kernel<F, SUB>: prefill_variant 0 / 1 (both page sizes)
    [_v(f"ap-{dt}-sub{sub}", f, PAGE16 + PAGE32, prefill_variant=sub - 1)
     for f, dt in ((False, "bf16"), (True, "fp8")) for sub in (1, 2)] +
    # attn_prefill2_kernel
    [_v("ap2-bf16-lean-wpg", False, PAGE16 + ("ragged12x3",)),  # the default bf16 route
     _v("ap2-bf16-lean", False, PAGE16, prefill_wpg=0),
     _v("ap2-fp8-lean", True, PAGE16, prefill_fp8_mfma=0),
     _v("ap2-fp8-lean-hkv3", True, ("ragged12x3",)),  # default knobs: hkv = 3 is no power of two
     _v("ap2-bf16-p32", False, PAGE32),  # non-LEAN: the routed page-32 kernel
     _v("ap2-fp8-p32", True, PAGE32),
     _v("ap2-bf16-v5", False, PAGE16, prefill_variant=5),  # non-LEAN at page 16
     _v("ap2-fp8-v5", True, PAGE16, prefill_variant=5)] +
    # attn_prefill8_kernel: 1 is the default fp8 route
    [_v(f"ap8-mfma{m}", True, PAGE16, prefill_fp8_mfma=m) for m in range(1, 9)] +
    # paged_attn_kernel<2, F>
    [_v(f"pa2-{dt}-ns{ns}", f, SPLIT, nqt=2, nsplit=ns)
     for f, dt in ((False, "bf16"), (True, "fp8")) for ns in (1,) + pp.NSPLITS]
)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from chronos import ops

    ops.load()
    import chronos.native as n

    assert "_C" in n._loaded, "HIP kernel library must be the one running"
    yield
    for name in KNOBS:
        torch.ops.chronos.set_knob(name, -1)


@pytest.fixture(autouse=True)
def _stop_after_device_error():
    """A device error is sticky for the process: end the session there rather than launch the remaining probes."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further launches: {e}", returncode=3)


@contextlib.contextmanager
def knobs(**kw):
    """Set the knobs for the block; erase the overrides afterwards (set_knob(name, -1)) whatever happens."""
    assert set(kw) <= set(KNOBS)
    try:
        for name, v in kw.items():
            torch.ops.chronos.set_knob(name, v)
        yield
    finally:
        for name in kw:
            torch.ops.chronos.set_knob(name, -1)


@functools.lru_cache(maxsize=None)
def gpu_args(shape, kind, fp8, nqt):
    """The probe's launch arguments on the device (uploaded once; the CPU probe keeps the closed form)."""
    from chronos import ops

    p = pp.probe(shape, kind, fp8)
    tiles = ops.attention_tiles(p.q_lens, p.hq, p.hkv, nqt)
    tt = torch.tensor(tiles, dtype=torch.int32, device=DEV).view(-1, 2)
    return tuple(x.to(DEV) for x in (p.q, p.k, p.v, p.bt, p.qs, p.ctx)) + (tt, len(tiles))


def attend(p, shape, nqt, nsplit):
    from chronos import ops

    q, k, v, bt, qs, ctx, tt, nt = gpu_args(shape, p.kind, p.fp8, nqt)
    ks, vs = p.scales
    k0, v0 = k.clone(), v.clone()
    out = ops.paged_attention(q, k, v, bt, qs, ctx, tt, nt, nqt, nsplit, 1.0 / math.sqrt(128), ks, vs)
    torch.cuda.synchronize()
    assert torch.equal(k, k0) and torch.equal(v, v0), "paged_attention must not write the caches"
    return out


@pytest.mark.parametrize("kind", ["U", "C"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_prefill_probe(variant, kind):
    """One launch per shape of the variant's list.  ragged: q_lens [1, 17, 64, 5, 100, 33] on prefixes [0, 0, 136, 32,
    0, 1100] at hq / hkv = 32 / 8, 64 / 8, 16 / 1, 4 / 4 (a one-token sequence, a fresh prompt, prefixes that are no
    multiple of 16 or 64, partial last pages and tiles at every G, several tiles per sequence so the heaviest-first
    walk meets both orders, one context past the 1024-token window); g1_two_tiles: 128 tokens per tile, a tile with
    two valid rows, a ``wave_min_pos`` per wave; long_u (U only): a 200-token chunk on a 2000-token prefix under a block
    table wider than needed, its padding pointing at poison.  The nqt = 2 variants take the shapes whose comb also aims
    at the kv-split edges of every 32-row tile.

    Found by the C probe, fixed in attention_prefill.hip: ap8-mfma5 and ap8-mfma8 (attn_prefill8_kernel<PV8, !FOLD,
    MSUM>, A/B variants) failed every row whose class has no member among the first 64 keys — "1406 of 7040 (token,
    head) rows off ... seq 2 ctx 200 token 0 head 4 L 137: class 124 members [121]..121 (n 1, aimed at s 15): no
    one-key explanation ..., max err 7.385" — while U passed.  The non-FOLD rescale branch (``__any(mx > m +
    kRescaleThr)``) scaled ``lsum`` and ``o`` by alpha but not ``lacc``, the ones-MFMA row sums MSUM divides by: when
    the needle's 65 log2 units arrived in a later stage, O dropped the 64+ keys before it (alpha = 2^-65) and l kept
    counting them, so the output was the right sum over the wrong count.  Random K / V rarely moves the maximum by
    more than the threshold after the first stage, and then by a few per cent of l."""
    fails = []
    for shape in variant["shapes"]:
        if kind not in pp.SHAPES[shape][1]:
            continue
        p = pp.probe(shape, kind, variant["fp8"])
        with knobs(**variant["knobs"]):
            out = attend(p, shape, variant["nqt"], variant["nsplit"])
        if bool(pp.violations(out, p).any()):
            fails.append(f"{shape}: " + pp.signature(out, p))
    assert not fails, f"{kind} probe\n" + "\n".join(fails)
