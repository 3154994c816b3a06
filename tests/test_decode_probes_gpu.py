"""Exact per-key probes (tests/_decode_probes.py) through every decode-attention instantiation that
``launch_paged_attn`` and ``launch_decode_attn_rope`` (csrc/kernels/attention.hip) can dispatch.

U (uniform: K = 0, one-hot V) says which keys were attended, N (needle keys, position-coded V) says which V went with
which K; poison around every context says what was read that should not have been.  The bounds are derived in
tests/_decode_probes.py (2^-7 relative: the bf16 store's 2^-8, twice under the cascade) — one wrong key among 4096 is
four times outside them.  A failure prints the probe's signature: the dims off and by how many counts (U), or the position
whose code row came back (N).

Instantiation -> how it is selected -> test (U and N each; knobs are set for the call and erased again):

  paged_decode_kernel<F, PF, LEAN, OCC, RP, KL>: launch_paged_attn's first branch (tiles == nullptr, nqt 1, nsplit 1,
  max_q 1, nitems >= decode_min_items)
    <F, 0, 1, 3>                 the default (bf16: KLDS)              test_one_wave_default, test_one_wave_small_batches
    <F, 1, 0, 1>                 ``if (pf) PD_LAUNCH``                 test_one_wave_variants[*-pf1-*]
    <F, 0, L, 3>, <F, 0, L, 1>   PD_OCC ``else if (occ3)`` / ``else``  test_one_wave_variants[*-pf0-lean{L}-occ3{1,0}-klds1-*]
    <bf16, 0, L, 3, 0, KL = 0>   PD_OCC ``!F && !klds && occ3``        test_one_wave_variants[bf16-pf0-lean{L}-occ31-klds0-*]
  paged_decode_kernel<bf16, 0, 1, OCC, RP = 1, KL>: launch_decode_attn_rope
    <.., 3, 1, KL = 0>           ``!knob("decode_klds")``              test_fused_rope[*-klds0-*]
    <.., 3, 1>, <.., 1, 1>       ``decode_occ3`` / ``else``            test_fused_rope[occ31-klds1-*], [occ30-klds1-*]
  casc_prefix_kernel<true> and the merge         ``casc != nullptr``   test_cascade
  paged_attn_kernel<1, F>        PA_LAUNCH, ``!pf1``                   test_split_over_waves_no_split (fewer items than
                                 decode_min_items; decode_attn_legacy -> ``goto legacy``), test_paged_attn_split[*-pf0-*]
  paged_attn_kernel<1, F, true>  PA_LAUNCH, ``pf1``                    test_paged_attn_split[*-pf1-*] (split_lds = 0)
  split_decode_kernel<bf16, 1 | 2>, <fp8, 2 | 3 | 4>   SD_LAUNCH (nsplit > 1 && split_lds, or max_q > 1)
                                                                       test_split_decode, test_split_decode_multi_token
  paged_attn_combine_kernel<1>   ``nsplit > 1 && cnt == nullptr``      test_paged_attn_split[*-ns16-cap4], [*-ns3-cap2],
                                 test_split_decode[*-ns16-comb1], [*-ns4-comb0], test_split_decode_multi_token
"""
import contextlib
import functools
import itertools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _decode_probes as dp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = 1.0 / math.sqrt(128)
KNOBS = ("decode_pf", "decode_lean", "decode_occ3", "decode_klds", "decode_min_items", "decode_attn_legacy",
         "split_lds", "split_lds_nb", "split_pf", "attn_inkernel_combine", "sd_inkernel_max_split",
         "inkernel_combine_max_split")


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
def gpu_probe(shape, kind, fp8=False):
    return dp.probe(shape, kind, fp8).to(DEV)


def attend(p, nsplit=1):
    from chronos import ops

    ks, vs = p.scales
    k0, v0 = p.k.clone(), p.v.clone()
    out = ops.paged_attention(p.q, p.k, p.v, p.bt, p.qs, p.ctx, None, p.B, 1, nsplit, None, ks, vs, max_q=p.max_q)
    torch.cuda.synchronize()
    assert torch.equal(p.k, k0) and torch.equal(p.v, v0), "paged_attention must not write the caches"
    return out


def _dt(fp8):
    return "fp8" if fp8 else "bf16"


FP8 = pytest.mark.parametrize("fp8", [False, True], ids=_dt)
KIND = pytest.mark.parametrize("kind", ["U", "N"])


# ---- one wave per (sequence, kv head), >= 1024 items ---------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wave32x8", "wave64x8"])
@KIND
@FP8
def test_one_wave_default(shape, kind, fp8):
    """136 sequences x 8 kv heads = 1088 items at the default knobs: paged_decode_kernel<F, false, true, 3> (KLDS for
    bf16) by ``PD_OCC``'s ``else if (occ3)``.  Contexts of 1 .. 4+ steps of 32 tokens, both sides of every step edge,
    1023 / 1024 / 1025 (the 64-entry block-table window refill) and past it."""
    p = gpu_probe(shape, kind, fp8)
    assert p.B * p.hkv >= 1024
    dp.check(attend(p), p, "one-wave default")


WAVE_VARIANTS = [(False, *v) for v in itertools.product((0, 1), repeat=4)] + \
                [(True, *v, 1) for v in itertools.product((0, 1), repeat=3)]  # fp8 ignores decode_klds


@pytest.mark.parametrize("shape", ["wave32x8", "wave64x8"])
@KIND
@pytest.mark.parametrize("fp8,pf,lean,occ3,klds", WAVE_VARIANTS,
                         ids=[f"{_dt(v[0])}-pf{v[1]}-lean{v[2]}-occ3{v[3]}-klds{v[4]}" for v in WAVE_VARIANTS])
def test_one_wave_variants(shape, kind, fp8, pf, lean, occ3, klds):
    """Every compiled variant of the one-wave kernel on test_one_wave_default's inputs: decode_pf (two register sets,
    <F, true, false, 1>), decode_lean, decode_occ3 (OCC 3 / 1) and decode_klds = 0 (bf16: K straight to VGPRs,
    <.., KL = false>, taken only with occ3)."""
    p = gpu_probe(shape, kind, fp8)
    with knobs(decode_pf=pf, decode_lean=lean, decode_occ3=occ3, decode_klds=klds):
        out = attend(p)
    dp.check(out, p, f"one-wave pf={pf} lean={lean} occ3={occ3} klds={klds}")


# ---- the one-wave kernel at small batches --------------------------------------------------------------------------
SMALL = [s for s in dp.SHAPES if s.startswith("g")]


@pytest.mark.parametrize("shape", SMALL)
@KIND
@FP8
def test_one_wave_small_batches(shape, kind, fp8):
    """decode_min_items = 1 routes a handful of sequences to paged_decode_kernel: G = 1, 4 and 16; nitems % 4 = 1, 2, 3
    (the whole-wave early return ``item >= nitems`` in a partly filled workgroup); block tables 1 and 3 entries wide
    (``lane < bt_stride``)."""
    p = gpu_probe(shape, kind, fp8)
    assert p.bt.shape[1] in (1, 3)
    with knobs(decode_min_items=1):
        out = attend(p)
    dp.check(out, p, f"one-wave small batch {shape}")


# ---- fused RoPE + KV write -----------------------------------------------------------------------------------------
def fused(p, casc=None):
    """ops.decode_attention_rope on fresh copies of the probe's pre-call caches -> (out, k, v)."""
    from chronos import ops

    k, v = p.k_pre.clone(), p.v_pre.clone()
    out = ops.decode_attention_rope(p.qkv, p.pos, p.cos_sin, k, v, p.bt, p.ctx, p.B, p.hq, SCALE, casc)
    torch.cuda.synchronize()
    return out, k, v


def check_kv_written(p, k, v):
    """The caches after the call hold the new K / V: against ref.rope_kv_write as test_kernels_gpu does (K 1e-2 + 1e-2
    relative: RoPE rounding may differ by an fma contraction; V equal)."""
    d = (k.float() - p.k.float()).abs()
    assert bool((d <= 1e-2 + 1e-2 * p.k.float().abs()).all()), f"K cache max err {float(d.max()):.4g}"
    assert torch.equal(v, p.v), "V cache differs from rope_kv_write"


@pytest.mark.parametrize("shape", ["rope32x8", "rope8x2_b7", "rope16x1_b5"])
@KIND
@pytest.mark.parametrize("klds", [1, 0], ids=["klds1", "klds0"])
@pytest.mark.parametrize("occ3", [1, 0], ids=["occ31", "occ30"])
def test_fused_rope(shape, kind, klds, occ3):
    """paged_decode_kernel<false, false, true, OCC, RP = true, KL> through ops.decode_attention_rope: 1040 items at the
    default threshold, and 5 / 7 sequences with decode_min_items = 1.  The new token sits at every block offset 0..15
    and on both sides of a 32-token step and of the 1024-token window; its cache slot is poisoned before the call (a
    stale read shows).  N: needles at the new token (raw k = 4 raw q: pins the parked-K copy into the step's LDS tile)
    and at older positions (cache K = 4 x the reference-roped q)."""
    p = gpu_probe(shape, kind)
    small = p.B * p.hkv < 1024
    if small:
        out, _, _ = fused(p)
        assert out is None, "below decode_min_items the fused op must decline"
    with knobs(decode_klds=klds, decode_occ3=occ3, **({"decode_min_items": 1} if small else {})):
        out, k, v = fused(p)
        with knobs(decode_attn_legacy=1):
            assert fused(p)[0] is None, "decode_attn_legacy must turn the fused op off"
    assert out is not None, "the fused one-wave kernel must serve this launch"
    check_kv_written(p, k, v)
    dp.check(out, p, f"fused rope klds={klds} occ3={occ3}")


# ---- cascade -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["casc1", "casc3"])
@pytest.mark.parametrize("kind", ["U", "N", "N1"])
def test_cascade(shape, kind):
    """casc_prefix_kernel<true> + the merge in paged_decode_kernel<.., RP = true>: P = 1 and 3 shared prefix blocks, 132
    sequences; every fourth has ctx <= 16 P and is not a member.  Members' suffix walks start at 16 P (P odd: the
    32-token step grid is offset by 16).  N / N1: half of the heads' needles inside the prefix (first key, last key of
    the prefix), the others from token 16 P and 16 P + 1 on; N1 swaps the halves."""
    p = gpu_probe(shape, kind)
    P = len(p.casc)
    casc = torch.tensor([P] + p.casc + [0] * (8 - P), dtype=torch.int32, device=DEV)
    co = torch.full((p.B, p.hq, 128), float("nan"), dtype=torch.bfloat16, device=DEV)
    cl = torch.full((p.B, p.hq), float("nan"), dtype=torch.float32, device=DEV)
    out, k, v = fused(p, (casc, co, cl))
    assert out is not None
    member = p.ctx > 16 * P
    assert bool(member.any()) and bool((~member).any())
    # routing: the producer wrote exactly the member rows
    assert not bool(torch.isnan(cl[member]).any()) and bool(torch.isnan(cl[~member]).all())
    check_kv_written(p, k, v)
    dp.check(out, p, f"cascade P={P}")


# ---- the split-over-waves kernel without a split -------------------------------------------------------------------
@KIND
@FP8
def test_split_over_waves_no_split(kind, fp8):
    """paged_attn_kernel<1, F> (PA_LAUNCH, ``!pf1``: nsplit == 1): 12 sequences x 8 kv heads = 96 items, fewer than
    decode_min_items = 1024; and test_one_wave_default's 1088 items with decode_attn_legacy = 1 (``goto legacy``)."""
    p = gpu_probe("legacy12", kind, fp8)
    assert p.B * p.hkv < 1024
    dp.check(attend(p), p, "paged_attn_kernel<1> small batch")
    p = gpu_probe("wave32x8", kind, fp8)
    with knobs(decode_attn_legacy=1):
        out = attend(p)
    dp.check(out, p, "paged_attn_kernel<1> decode_attn_legacy")


# ---- the LDS-staged split kernel -----------------------------------------------------------------------------------
SD_NB = [(False, 1), (False, 2), (True, 2), (True, 3), (True, 4)]  # every ring depth compiled per dtype
SD_NB_IDS = [f"{_dt(f)}-nb{nb}" for f, nb in SD_NB]
# (nsplit, attn_inkernel_combine): in-launch combine (nsplit <= sd_inkernel_max_split = 4) and the separate kernel
SD_SPLITS = [(2, 1), (4, 1), (4, 0), (16, 1)]


@pytest.mark.parametrize("nsplit,comb", SD_SPLITS, ids=[f"ns{n}-comb{c}" for n, c in SD_SPLITS])
@KIND
@pytest.mark.parametrize("fp8,nb", SD_NB, ids=SD_NB_IDS)
def test_split_decode(fp8, nb, kind, nsplit, comb):
    """split_decode_kernel<F, NB> (SD_LAUNCH: nsplit > 1 && split_lds): contexts 1 .. 4096, so splits with no key
    (ctx < 32 nsplit), partial last steps and 1 .. 8 steps per wave (every ring phase); N holds the last key of one
    split and the first of the next for nsplit 2, 3, 4 and 16."""
    p = gpu_probe("split32x8", kind, fp8)
    with knobs(split_lds_nb=nb, attn_inkernel_combine=comb):
        out = attend(p, nsplit)
    dp.check(out, p, f"split_decode nb={nb} nsplit={nsplit} comb={comb}")


@pytest.mark.parametrize("shape", ["mq4_8x2", "mq4_4x1", "mq2_8x2", "mq2_4x1"])
@KIND
@pytest.mark.parametrize("fp8,nb", SD_NB, ids=SD_NB_IDS)
def test_split_decode_multi_token(shape, fp8, nb, kind):
    """Multi-token decode (max_q 4 and 2, G x max_q <= 16) always takes split_decode_kernel (``max_q > 1``), nsplit 1
    included: token j of an n-token chunk attends ctx - (n - 1 - j) keys (U counts them; N gives every (token, head)
    column its own needle, the last key it may see among them)."""
    p = gpu_probe(shape, kind, fp8)
    assert p.max_q == int(shape[2]) and p.max_q * (p.hq // p.hkv) <= 16
    fails = []
    for nsplit, comb in [(1, 1)] + SD_SPLITS:
        with knobs(split_lds_nb=nb, attn_inkernel_combine=comb):
            out = attend(p, nsplit)
        if bool(dp.violations(out, p).any()):
            fails.append(f"nsplit={nsplit} comb={comb}: " + dp.signature(out, p))
    assert not fails, "\n".join(fails)


# ---- the split-over-waves kernel under a split ---------------------------------------------------------------------
PA_SPLITS = [(3, 4), (16, 4), (3, 2)]  # (nsplit, inkernel_combine_max_split): in-launch, separate, separate by the cap


@pytest.mark.parametrize("nsplit,cap", PA_SPLITS, ids=[f"ns{n}-cap{c}" for n, c in PA_SPLITS])
@pytest.mark.parametrize("pf", [1, 0], ids=["pf1", "pf0"])
@KIND
@FP8
def test_paged_attn_split(fp8, kind, pf, nsplit, cap):
    """paged_attn_kernel<1, F, PF> (PA_LAUNCH) under a kv split with split_lds = 0: split_pf = 1 -> <1, F, true>
    (``pf1``), 0 -> <1, F>; the last split's in-launch combine (nsplit 3 <= inkernel_combine_max_split) and
    paged_attn_combine_kernel<1> (nsplit 16, or the cap lowered to 2)."""
    p = gpu_probe("split32x8", kind, fp8)
    with knobs(split_lds=0, split_pf=pf, inkernel_combine_max_split=cap):
        out = attend(p, nsplit)
    dp.check(out, p, f"paged_attn split pf={pf} nsplit={nsplit} cap={cap}")
