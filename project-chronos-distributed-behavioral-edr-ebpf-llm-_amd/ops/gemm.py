"""Projection GEMMs.

``linear(x, w)`` computes ``x @ w.T`` for weights stored [out, in] (HF layout); ``gate_up_silu`` is the fused K8+K9 and
``gemv_resid`` the O / down producer with the residual add + RMSNorm partial sums as its epilogue (-> ResidOut).  All
three are one dispatcher, ``_project``, which walks one ladder by weight kind and then by measured shape:

* MXFP4 weights (a Q4Tensor): the W4A16 GEMV (csrc/kernels/gemv.hip W4) at M = 1 (``W4_MAX_M``); the W4A16 mode of the
  skinny kernel (csrc/kernels/gemm_skinny.hip) at M = 2-64 where ``gemm_plan.json`` "w4plans" records it faster than
  the bf16 route by more than 3 % (``scripts/bench_skinny_w4.py``); the fused W4A16 MFMA GEMM
  (csrc/kernels/gemm_w4m.hip) at M = 65-512 where "w4mplans" records a win (``scripts/bench_mid_w4.py``): over the bf16
  kernel on the copy (both modes) or only over expansion + that kernel (packed-only tensors).  Everything else runs
  the bf16 steps below on ``w4_dense(w)``: the resident copy, or for a packed-only Q4Tensor (no copy) a scratch that
  one ``w4_expand`` launch (csrc/kernels/w4_expand.hip) fills in front of the GEMM, the same bits as the copy.  A
  packed-only tensor takes the skinny kernel on every M <= 64 shape it accepts (``w4_plan(packed=True)``);
* fp8 weights (a QTensor): the W8A16 GEMV at its shapes (M <= 4; the fused norm and the residual producer: M <= 2),
  else the activations are quantised and the W8A8 op runs (``ops.qlinear``, routed by "qplans").  Only for a caller
  that asks with ``a16=True`` (the model in a W8A16 step above two rows, ``LlamaModel.w8a16_rows``), a call the GEMV
  does not take goes to the W8A16 mode of the skinny kernel (gemm_skinny.hip WM = kW8, M <= 64: e4m3 bytes converted
  in registers, bf16 activations, the bf16 family's fused norm / SwiGLU / residual epilogues, no quantisation launch)
  where ``w8_plan`` has a route: a winning row of "w8plans" (``scripts/bench_skinny_w8.py``), or under
  CHRONOS_W8_SKINNY=model the cost-model pick; without a route it is the W8A8 op as before.  Default calls never ask;
* bf16 weights, M <= ``GEMV_MAX_M`` (1: single-stream decode): the hand-written GEMV (csrc/kernels/gemv.hip), 1 KiB
  row-contiguous weight streaming — beats hipBLASLt on every decode shape;
* bf16 weights above: the hand-written MFMA GEMM families with their fused epilogues — the residual epilogue, the
  folded RMSNorm of a LazyNorm input as a per-row scale, SwiGLU on gate_up: the skinny-M weight-streaming kernel
  (M <= 128: jump-forward forwards, tail decode buckets) and the tile GEMMs (csrc/kernels/gemm_pp.hip, gemm_lg.hip)
  above, with the kernel, tile config and split-K of the measured plan (``gemm_plan.json`` "plans": per (N, K,
  epilogue) the best by M range, from ``scripts/tune_gemm_pp.py`` on one MI355X, random operands, cold weights; plan
  cfg >= 100 is skinny config cfg - 100);
* hipBLASLt (torch.matmul) only where the plan records that the library wins by more than 3 % (the "plain library
  GEMM" rule), for shapes the kernels do not take (K % 64, N % 4) and for ``linear(out=)``.  CHRONOS_PP=lib|own|auto
  forces a side.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import torch

# Largest M routed to the GEMV (gemv_ok).  Env CHRONOS_GEMV_MAX_M; scripts/single_stream.py A/Bs it (py_gemv_max_m).
# M = 2 goes to the skinny MFMA GEMM: the two-row GEMV streams at 1-3.5 TB/s against 4-5.5 at M = 1 and the skinny
# kernel's 3.4-4.9 at M = 3 (profiles/r3_gemm_table.md).
GEMV_MAX_M = int(os.environ.get("CHRONOS_GEMV_MAX_M", "1"))

# ---- the batched GEMM family (gemm_pp.hip) ----------------------------------------------------------------------
PP_MODE = os.environ.get("CHRONOS_PP", "auto")  # auto | own | lib
PP_PLAIN, PP_SWIGLU, PP_RESID = 0, 1, 2
# x rows (BM) / W rows (BN) per tile.  0-11: gemm_pp.hip (ping-pong); 12-35: gemm_lg.hip (software-pipelined: 12-19 and
# 29-31 the ring schedule, 20-28 the 64-deep slab schedule, 32-39 mid-M weight streaming with 64 W rows, 72-75 the
# same for M <= 32 with 32-row x tiles; 76-77 192 W rows x 128 x rows; 78-79 32-row x tiles with 7 / 12-stage rings;
# 80 = 20 on 32x32x16 MFMAs; 81-89 the 4-wave HB slab loop, 256 x 256 tiles, no split-K: 86 / 87 precomputed addressing
# (87: hipBLASLt's DMA distribution), 88 / 89 the same + the LDS-staged epilogue, 90 = 88 with the next slab's
# fragment reads from MFMA 94)
_PP_BM = {0: 256, 1: 128, 2: 256, 3: 128, 4: 256, 5: 128, 6: 256, 7: 128, 8: 256, 9: 128, 10: 256, 11: 128,
          12: 256, 13: 128, 14: 256, 15: 128, 16: 256, 17: 128, 18: 256, 19: 128, 20: 256, 21: 256, 22: 128, 23: 128,
          24: 256, 25: 128, 26: 256, 27: 128, 28: 128, 29: 128, 30: 256, 31: 128, 32: 128, 33: 64, 34: 128, 35: 256,
          36: 64, 37: 128, 38: 64, 39: 64, 72: 32, 73: 32, 74: 32, 75: 32, 76: 128, 77: 128, 78: 32, 79: 32, 80: 256,
          **{c: 256 for c in range(81, 95)}}
_PP_BN = {0: 256, 1: 256, 2: 128, 3: 128, 4: 256, 5: 256, 6: 128, 7: 128, 8: 256, 9: 256, 10: 128, 11: 128,
          12: 256, 13: 256, 14: 128, 15: 128, 16: 256, 17: 256, 18: 128, 19: 128, 20: 256, 21: 256, 22: 256, 23: 128,
          24: 256, 25: 256, 26: 256, 27: 256, 28: 128, 29: 256, 30: 128, 31: 128, 32: 64, 33: 64, 34: 64, 35: 64, 36: 64, 37: 64, 38: 128, 39: 64, 72: 64, 73: 128, 74: 64, 75: 128, 76: 192, 77: 192, 78: 128, 79: 64, 80: 256,
          **{c: 256 for c in range(81, 95)}}
HB_FIRST, HB_LAST = 81, 94  # gemm_lg.hip HB configs (91: the 32x32x16 MFMA form; 92 / 93: 88 / 89 + square order;
# 94: 92 + the set-0 reads from MFMA 94)
HB_SPLITK = (88, 89, 90, 91, 92, 93, 94)  # ... with the staged epilogue: the only ones with a split-K path
LG_FIRST = 12  # first gemm_lg.hip config: kResid partials every BN/2 columns (gemm_pp: BN/4)
# relative per-CU MAC rate of each tile config at full occupancy (gate_up M = 1024 / 16384 sweeps, profiles/r3_gemm_pp_*,
# profiles/r4_gemm_lg_*)
_PP_RATE = {0: 1.0, 1: 0.84, 2: 0.84, 3: 0.66, 4: 1.0, 5: 0.71, 6: 0.73, 7: 0.6, 8: 1.0, 9: 0.84, 10: 0.84, 11: 0.66,
            12: 0.95, 13: 0.7, 14: 0.7, 15: 0.75, 16: 0.98, 17: 0.7, 18: 0.7, 19: 0.75, 20: 1.05, 21: 0.7, 22: 0.7,
            23: 0.75, 24: 1.1, 25: 0.8, 26: 1.1, 27: 0.8, 28: 0.75, 29: 0.8, 30: 0.8, 31: 0.75, 32: 0.5,
            33: 0.4, 34: 0.5, 35: 0.55, 36: 0.4, 37: 0.5, 38: 0.5, 39: 0.4, 72: 0.3,
            73: 0.3, 74: 0.3, 75: 0.3, 76: 0.75, 77: 0.7, 78: 0.3, 79: 0.3, 80: 1.05,
            **{c: 1.15 for c in range(81, 95)}}
# skinny-M configs (gemm_skinny.hip SK_CONFIGS): plan id SK_BASE + c -> (RT: W tiles of 16 rows, MT: M <= 16 MT,
# NW: waves splitting K inside the workgroup)
SK_BASE = 100
_SK = {0: (1, 1, 16), 1: (2, 1, 8), 2: (4, 1, 4), 3: (2, 2, 8), 4: (4, 2, 4), 5: (2, 4, 4), 6: (4, 4, 4),
       7: (2, 8, 4), 8: (1, 2, 16), 9: (1, 4, 16), 10: (2, 4, 8), 11: (1, 1, 8)}
SKINNY_MAX_M = 128
# W4A16 mode of the same kernel (gemm_skinny.hip SK4_CONFIGS: mxfp4 q / e streamed, bf16 MFMA): own config ids ->
# (RT, MT, NW); the unit is 128 k, so K % (128 NW split-K) == 0.  M <= 64 (MT <= 4); above that, up to 512 rows, the
# mid-M kernel of its own file takes over (gemm_w4m.hip, ``_W4M`` / ``W4_MID`` below).
_SK4 = {0: (4, 1, 4), 1: (4, 1, 4), 2: (4, 1, 8), 3: (2, 1, 8), 4: (2, 1, 8), 5: (2, 1, 16), 6: (1, 1, 16),
        7: (4, 2, 4), 8: (2, 2, 8), 9: (4, 2, 8), 10: (4, 4, 4), 11: (2, 4, 8), 12: (2, 4, 4)}
W4_SKINNY_MAX_M = 64
# Which Q4Tensor calls above the fp4 GEMV's M take the W4A16 skinny kernel (env CHRONOS_W4_SKINNY): ``plan`` = the
# measured rows of gemm_plan.json "w4plans" (a shape with no row runs the bf16 copy), ``off`` = the copy everywhere,
# ``model`` = the ``_sk4_model`` pick for every valid shape (the tests' way to the kernel on unmeasured shapes, like
# CHRONOS_PP=own).  Like every switch here it may be assigned at run time: the plan cache is keyed by the switches.
W4_SKINNY = os.environ.get("CHRONOS_W4_SKINNY", "plan")
# Above 64 rows, up to W4M_MAX_M, a Q4Tensor call can take the mid-M W4A16 GEMM (gemm_w4m.hip W4M_CONFIGS: config id ->
# (WN: W rows per tile, XM: x rows per tile, ST: x ring stages); K % (128 split-K) == 0, N % WN == 0, SwiGLU
# F % (WN / 2) == 0, any M).  Env CHRONOS_W4_MID (``W4_MID``, assignable like W4_SKINNY; a switch of its own, so that
# W4_SKINNY = "model" keeps meaning what it meant): ``plan`` = the measured rows of gemm_plan.json "w4mplans", rows
# [measured M, cfg, split-K, beats] read like "w4plans" — beats 2: faster than the routed bf16 kernel on the resident
# copy, routed in both weight modes; beats 1: faster only than expansion + that kernel, routed for a packed-only tensor
# alone; cfg < 0: measured, lost to both; no row: never measured, the copy / the expansion exactly as before (unlike
# ``w4_plan(packed=True)`` the model pick is NOT substituted: an unmeasured mid-M kernel is not known to beat an
# expansion) — ``off`` = the copy / the expansion everywhere, ``model`` = the ``_w4m_model`` pick for every valid shape
# (the tests' way onto unmeasured shapes).  With beats = 1 rows the two weight modes run different kernels at those
# points (same tolerance against the reference), as they already do at M <= 64.
_W4M = {0: (64, 64, 4), 1: (128, 64, 4), 2: (64, 128, 4), 3: (128, 128, 4)}
W4M_MIN_M, W4M_MAX_M = W4_SKINNY_MAX_M + 1, 512
W4_MID = os.environ.get("CHRONOS_W4_MID", "plan")
# W8A16 mode of the same kernel (gemm_skinny.hip SK8_CONFIGS: e4m3 bytes + per-row scales streamed, bf16 MFMA): own
# config ids -> (RT, MT, NW); the unit is 64 k, so K % (64 NW split-K) == 0 like the bf16 mode, and M <= 64.
_SK8 = {0: (4, 1, 4), 1: (4, 1, 8), 2: (2, 1, 8), 3: (2, 1, 16), 4: (1, 1, 16), 5: (4, 2, 4), 6: (2, 2, 8),
        7: (4, 2, 8), 8: (4, 4, 4), 9: (2, 4, 8), 10: (2, 4, 4), 11: (1, 1, 8)}
W8_SKINNY_MAX_M = 64
# Which ``a16=True`` QTensor calls the W8A16 GEMV does not take go to that mode (env CHRONOS_W8_SKINNY): ``plan`` = the
# measured winning rows of gemm_plan.json "w8plans" only, ``off`` = none, ``model`` = the ``_sk8_model`` pick for every
# valid shape (the tests' way onto the kernel).  Assignable at run time like W4_SKINNY.  Calls without ``a16`` never
# look at it: what an fp8 weight launches by default is what it launched before the mode existed.
W8_SKINNY = os.environ.get("CHRONOS_W8_SKINNY", "plan")
# The measured plans: gemm_plan.json (env CHRONOS_GEMM_PLAN: another file) read once, section -> {(N, K, epilogue):
# rows sorted by M}.  ``_plan_cache`` holds the answers of the plan functions, keyed by every switch they depend on.
# ``_plan_table = None`` (or ``_reset_plans()``) makes the next lookup read the file again.
_PLAN_SECTIONS = ("plans", "qplans", "w4plans", "w4mplans", "w8plans")
_plan_table: Optional[dict] = None
_plan_cache: dict = {}


def _load_plans() -> dict:
    global _plan_table
    if _plan_table is None:
        import json

        override = os.environ.get("CHRONOS_GEMM_PLAN")
        path = override or os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_plan.json")
        try:
            with open(path) as fh:
                raw = json.load(fh)
        except FileNotFoundError:
            if override:  # an explicit A/B override that does not exist must not silently measure the library
                raise FileNotFoundError(f"CHRONOS_GEMM_PLAN={override!r}: no such plan file") from None
            raw = {}
        key = lambda k: tuple(int(v) for v in k.split(","))  # noqa: E731
        _plan_table = {sec: {key(k): rows for k, rows in raw.get(sec, {}).items()} for sec in _PLAN_SECTIONS}
    return _plan_table


def _reset_plans(**sections) -> None:
    """Forget the plan file and every cached answer; the next lookup reads the file again.  With sections given
    (``plans=``, ``qplans=``, ``w4plans=``, ``w4mplans=``, ``w8plans=``: tables keyed like the loaded ones) these stand in for the
    file, the others empty: the tests' way to inject rows."""
    global _plan_table
    assert set(sections) <= set(_PLAN_SECTIONS), sections
    _plan_table = {sec: sections.get(sec, {}) for sec in _PLAN_SECTIONS} if sections else None
    _plan_cache.clear()


def _plan_row(section: str, key: tuple, m: int, last_covers_above: bool = True):
    """The row of a shape that decides M: rows [measured M, ...] sorted by M, a measured M decides (previous M, M].
    Above the last row: that row, or (``last_covers_above`` False, "w4mplans") None = not measured.  No rows: None."""
    rows = _load_plans()[section].get(key)
    if not rows:
        return None
    return next((r for r in rows if m <= r[0]), rows[-1] if last_covers_above else None)


QLG_BASE = 10  # qplan code >= QLG_BASE: gemm_lg.hip's fp8 config (code - QLG_BASE), row [M, code, split-K]
QLG_GEO = {0: (128, 256), 1: (256, 128), 2: (128, 128), 3: (128, 128),  # fp8 config -> (x rows, W rows) per tile
           4: (256, 256)}  # 4: the HB slab loop on the 32x32x64 fp8 MFMA (gemm_lg.hip F8HB)


def qplan_route(m: int, n: int, k: int, swiglu: bool) -> Optional[tuple[int, int]]:
    """W8A8 fp8 projection route from ops/gemm_plan.json "qplans" (``scripts/tune_gemm_pp.py --fp8``), rows
    [measured M, code(, split-K)] per (N, K, swiglu) read like the bf16 plan's: code 0 = the library's fp8 GEMM, 1 =
    fp8.hip (qgemv / block-scaled MFMA qgemm), QLG_BASE + c = gemm_lg.hip fp8 config c.  None = not measured."""
    pick = _plan_row("qplans", (n, k, int(swiglu)), m)
    if pick is None:
        return None
    return int(pick[1]), int(pick[2]) if len(pick) > 2 else 1


def qplan_own(m: int, n: int, k: int, swiglu: bool) -> Optional[bool]:
    """True = a hand-written fp8 kernel (fp8.hip or gemm_lg.hip), False = the library, None = not measured."""
    r = qplan_route(m, n, k, swiglu)
    return None if r is None else r[0] != 0


def _skinny_valid(cfg: tuple, unit: int, m: int, n: int, k: int, mode: int, sk: int) -> bool:
    """gemm_skinny.hip's shape rules for a (RT, MT, NW) config whose K unit is ``unit`` (bf16: 64, W4A16: 128)."""
    rt, mt, nw = cfg
    if m > 16 * mt or k % (unit * nw * sk):
        return False
    return (rt % 2 == 0 and n % 2 == 0 and (n // 2) % (8 * rt) == 0) if mode == PP_SWIGLU else n % (16 * rt) == 0


def _sk_valid(c: int, m: int, n: int, k: int, mode: int, sk: int) -> bool:
    return _skinny_valid(_SK[c], 64, m, n, k, mode, sk)


def _sk_model(m: int, n: int, k: int, mode: int, cus: int = 256) -> Optional[tuple[int, int]]:
    """Cost-model pick of a skinny config: the narrowest x tile covering M, W tiles >= x tiles (x re-read bytes <=
    weight bytes), split-K until the grid covers the CUs twice."""
    best = None
    for c, (rt, mt, nw) in _SK.items():
        if m > 16 * mt or (mt > 1 and m <= 8 * mt):
            continue
        groups = (n // 2) // (8 * rt) if mode == PP_SWIGLU else n // (16 * rt)
        for sk in (1, 2, 4, 7, 8, 14, 16):
            if not _sk_valid(c, m, n, k, mode, sk):
                continue
            # a cross-workgroup split costs more than it hides (profiles/r3_gemm_table.md): only when the grid
            # would otherwise leave CUs idle; then the widest workgroups
            t = (sk > 1 and groups >= cus, rt < mt, -min(groups * sk, cus), sk, -nw, -rt)
            if best is None or t < best[0]:
                best = (t, (SK_BASE + c, sk))
    return best[1] if best else None


def _sk4_valid(c: int, m: int, n: int, k: int, mode: int, sk: int) -> bool:
    """The binding's rules for the W4A16 skinny mode (bindings.cpp gemm_skinny with ``we``)."""
    if c not in _SK4 or sk < 1 or m < 1 or k < 1 or k > (1 << 20):
        return False
    return _skinny_valid(_SK4[c], 128, m, n, k, mode, sk)


def _sk4_model(m: int, n: int, k: int, mode: int, cus: int = 256) -> Optional[tuple[int, int]]:
    """Cost-model pick of a W4A16 skinny config for a shape without a measured row: the narrowest x tile covering M,
    split-K only while the grid leaves CUs idle, then the widest W tile and the most waves."""
    best = None
    for c, (rt, mt, nw) in _SK4.items():
        if mt > 1 and m <= 8 * mt:
            continue
        groups = (n // 2) // (8 * rt) if mode == PP_SWIGLU else n // (16 * rt)
        for sk in (1, 2, 4, 7, 8):
            if not _sk4_valid(c, m, n, k, mode, sk):
                continue
            t = (sk > 1 and groups >= cus, -min(groups * sk, cus), sk, -rt, -nw, c)
            if best is None or t < best[0]:
                best = (t, (c, sk))
    return best[1] if best else None


def w4_plan(m: int, n: int, k: int, mode: int = PP_PLAIN, packed: bool = False) -> Optional[tuple[int, int]]:
    """(W4 config, split-K) of the W4A16 skinny kernel for a Q4Tensor projection at this shape, or None for the bf16
    copy.  ``plan``: gemm_plan.json "w4plans", rows [measured M, cfg, split-K] per (N, K, mode) read like "plans"
    (cfg < 0 = the copy measured faster; no row = never measured = the copy).

    ``packed`` (a Q4Tensor without the copy): the alternative is no longer a free resident copy but an expansion —
    a full write and re-read of the weight matrix in front of the bf16 kernel — so every shape the kernel accepts takes
    it: the plan's winning row where there is one, the ``_sk4_model`` pick for a shape without a row and for a row the
    copy won (by at most 13 %, QKV / gate_up at M = 40-64; scripts/bench_w4_expand.py measures those points)."""
    if not _W4A16_DECODE or W4_SKINNY == "off" or m < 1 or m > W4_SKINNY_MAX_M:
        return None
    key = ("w4", W4_SKINNY, packed, m, n, k, mode)
    hit = _plan_cache.get(key, False)
    if hit is not False:
        return hit
    out = None
    if W4_SKINNY == "model":
        out = _sk4_model(m, n, k, mode)
    else:
        pick = _plan_row("w4plans", (n, k, mode), m)
        if pick is not None and pick[1] >= 0:
            out = (int(pick[1]), int(pick[2]))
        if packed and (out is None or not _sk4_valid(out[0], m, n, k, mode, out[1])):
            out = _sk4_model(m, n, k, mode)
    if out is not None and not _sk4_valid(out[0], m, n, k, mode, out[1]):
        out = None
    _plan_cache[key] = out
    return out


def _sk8_valid(c: int, m: int, n: int, k: int, mode: int, sk: int) -> bool:
    """The binding's rules for the W8A16 skinny mode (bindings.cpp gemm_skinny with ``wscale``)."""
    if c not in _SK8 or sk < 1 or m < 1 or k < 1 or k > (1 << 20):
        return False
    return _skinny_valid(_SK8[c], 64, m, n, k, mode, sk)


def _sk8_model(m: int, n: int, k: int, mode: int, cus: int = 256) -> Optional[tuple[int, int]]:
    """Cost-model pick of a W8A16 skinny config for a shape without a measured row: the narrowest x tile covering M,
    split-K only while the grid leaves CUs idle, then the widest W tile and the most waves (``_sk4_model``'s order)."""
    best = None
    for c, (rt, mt, nw) in _SK8.items():
        if mt > 1 and m <= 8 * mt:
            continue
        groups = (n // 2) // (8 * rt) if mode == PP_SWIGLU else n // (16 * rt)
        for sk in (1, 2, 4, 7, 8):
            if not _sk8_valid(c, m, n, k, mode, sk):
                continue
            t = (sk > 1 and groups >= cus, -min(groups * sk, cus), sk, -rt, -nw, c)
            if best is None or t < best[0]:
                best = (t, (c, sk))
    return best[1] if best else None


def w8_plan(m: int, n: int, k: int, mode: int = PP_PLAIN) -> Optional[tuple[int, int]]:
    """(W8 config, split-K) of the W8A16 skinny kernel for an ``a16`` QTensor projection at this shape, or None for
    today's route (W8A8).  ``plan``: gemm_plan.json "w8plans", rows [measured M, cfg, split-K] per (N, K, mode) read
    like "w4plans" (cfg < 0 = measured and lost; no row = never measured: both None)."""
    if W8_SKINNY == "off" or m < 1 or m > W8_SKINNY_MAX_M:
        return None
    key = ("w8", W8_SKINNY, m, n, k, mode)
    hit = _plan_cache.get(key, False)
    if hit is not False:
        return hit
    out = None
    if W8_SKINNY == "model":
        out = _sk8_model(m, n, k, mode)
    else:
        pick = _plan_row("w8plans", (n, k, mode), m)
        if pick is not None and pick[1] >= 0:
            out = (int(pick[1]), int(pick[2]))
    if out is not None and not _sk8_valid(out[0], m, n, k, mode, out[1]):
        out = None
    _plan_cache[key] = out
    return out


def _w4m_valid(c: int, m: int, n: int, k: int, mode: int, sk: int) -> bool:
    """The binding's rules for the mid-M W4A16 GEMM (bindings.cpp gemm_w4m)."""
    if c not in _W4M or sk < 1 or m < 1 or k < 1 or k > (1 << 20) or m * k >= (1 << 30) or n < 1:
        return False
    wn = _W4M[c][0]
    if k % (128 * sk):
        return False
    return (n % 2 == 0 and (n // 2) % (wn // 2) == 0) if mode == PP_SWIGLU else n % wn == 0


def _w4m_model(m: int, n: int, k: int, mode: int, cus: int = 256) -> Optional[tuple[int, int]]:
    """Cost-model pick of a mid-M W4A16 config for a shape without a measured row: the x tile with the fewest padded
    rows (then the wider one), split-K while the grid leaves CUs idle and a slice keeps at least a ring of stages, and
    the wide W tile (half the x re-reads) only where its grid still covers the CUs."""
    best = None
    for c, (wn, xm, st) in _W4M.items():
        tm = -(-m // xm)
        tiles = tm * ((n // 2) // (wn // 2) if mode == PP_SWIGLU else n // wn)
        for sk in (1, 2, 4, 7, 8):
            if not _w4m_valid(c, m, n, k, mode, sk) or (sk > 1 and k // (128 * sk) < st):
                continue
            grid = tiles * sk
            t = (tm * xm - m, -xm, sk > 1 and tiles >= cus, -min(grid, cus), sk, -wn, c)
            if best is None or t < best[0]:
                best = (t, (c, sk))
    return best[1] if best else None


def w4m_plan(m: int, n: int, k: int, mode: int = PP_PLAIN, packed: bool = False) -> Optional[tuple[int, int]]:
    """(config, split-K) of the mid-M W4A16 GEMM (gemm_w4m.hip) for a Q4Tensor projection at this shape, or None for
    the bf16 route (the copy, or the expansion when ``packed``).  See ``W4_MID`` above for the plan's semantics."""
    if not _W4A16_DECODE or W4_MID == "off" or m < W4M_MIN_M or m > W4M_MAX_M:
        return None
    key = ("w4m", W4_MID, packed, m, n, k, mode)
    hit = _plan_cache.get(key, False)
    if hit is not False:
        return hit
    out = None
    if W4_MID == "model":
        out = _w4m_model(m, n, k, mode)
    else:
        pick = _plan_row("w4mplans", (n, k, mode), m, last_covers_above=False)  # no row at or above M: not measured
        if pick is not None and pick[1] >= 0 and (pick[3] >= 2 or (pick[3] == 1 and packed)):
            out = (int(pick[1]), int(pick[2]))
    if out is not None and not _w4m_valid(out[0], m, n, k, mode, out[1]):
        out = None
    _plan_cache[key] = out
    return out


def _pp_valid(cfg: int, n: int, k: int, mode: int, sk: int, m: int = 0) -> bool:
    if cfg >= SK_BASE:
        return cfg - SK_BASE in _SK and _sk_valid(cfg - SK_BASE, m, n, k, mode, sk)
    bn = _PP_BN[cfg]
    if k % 64 or (k // 64) % sk or (HB_FIRST <= cfg <= HB_LAST and sk != 1 and cfg not in HB_SPLITK):
        return False
    return n % 4 == 0 if mode == PP_PLAIN else n % bn == 0


def _pp_model(m: int, n: int, k: int, mode: int, cus: int = 256) -> tuple[int, int]:
    """Cost-model pick for a shape the measured plan does not list: whole rounds of tiles over the CUs at each
    config's per-CU rate, plus the split-K slab traffic."""
    best, arg = None, (0, 1)
    for cfg in (0, 1, 2, 3):
        bm, bn = _PP_BM[cfg], _PP_BN[cfg]
        tiles = -(-m // bm) * -(-n // bn)
        for sk in (1, 2, 4):
            if not _pp_valid(cfg, n, k, mode, sk) or (sk > 1 and tiles * sk > 2 * cus):
                continue
            rounds = -(-tiles * sk // cus)
            t = rounds * bm * bn * (k // sk) / _PP_RATE[cfg] / 256.0 ** 2 + (sk > 1) * tiles * sk * bm * bn * 4 / 5e5
            if best is None or t < best:
                best, arg = t, (cfg, sk)
    return arg


def pp_plan(m: int, n: int, k: int, mode: int = PP_PLAIN) -> Optional[tuple[int, int]]:
    """(config, split-K) of the hand-written batched GEMM for this shape — config >= SK_BASE is the skinny kernel —
    or None for the library."""
    if m <= GEMV_MAX_M or PP_MODE == "lib":
        return None
    key = ("pp", PP_MODE, m, n, k, mode)
    hit = _plan_cache.get(key, False)
    if hit is not False:
        return hit
    out = None
    if k % 64 == 0 and (n % 4 == 0 if mode == PP_PLAIN else n % 128 == 0):
        if PP_MODE == "own":
            out = (_sk_model(m, n, k, mode) if m <= SKINNY_MAX_M else None) or _pp_model(m, n, k, mode)
        else:
            # rows [measured M, cfg, split-K]: the last row also decides everything above it.  cfg < 0 = the library
            # measured faster.
            pick = _plan_row("plans", (n, k, mode), m)
            if pick is not None and pick[1] >= 0:
                out = (pick[1], pick[2])
        # auto, shape never measured: the library (a hand-written config is routed only on a recorded A/B)
        if out is not None and not _pp_valid(out[0], n, k, mode, out[1], m):
            out = None
    _plan_cache[key] = out
    return out


def pp_gemm(x: torch.Tensor, w: torch.Tensor, mode: int, plan: tuple[int, int], resid=None, part=None,
            eps: float = 1e-5):
    """One launch of gemm_pp.hip (or gemm_skinny.hip for a skinny plan): returns (y, partials) — partials only for
    the residual epilogue."""
    from . import _k

    k = x.shape[-1]
    if plan[0] >= SK_BASE:
        return _k().gemm_skinny(x.reshape(-1, k), w, mode, plan[0] - SK_BASE, plan[1], resid, part, eps)
    y, pt = _k().gemm_pp(x.reshape(-1, k), w, mode, plan[0], plan[1], resid, part, eps, False)
    return y, pt


@dataclass
class ResidOut:
    """Output of a decode producer GEMV with the residual epilogue (``gemv_resid``): the new residual stream
    ``s = bf16(bf16(x @ w.T) + resid)`` and the per-workgroup partial sums of s^2 the next RMSNorm needs."""
    s: torch.Tensor
    part: torch.Tensor


@dataclass
class LazyNorm:
    """``rmsnorm(s) * w`` of a residual stream a ResidOut producer just wrote, not computed yet.

    Only built for models whose norm weights are folded into the consuming projections (``w`` is then ones).  A decode
    GEMV consumer (``linear`` / ``gate_up_silu`` / the fused QKV projection) applies it as one per-row scale of its
    outputs (csrc/kernels/gemv.hip NORMP: inv from the producer's partials), so the norm costs no launch; any other
    consumer calls ``materialize`` (the standalone RMSNorm kernel: equal up to rounding)."""
    s: torch.Tensor
    part: torch.Tensor
    w: torch.Tensor
    eps: float
    _y: Optional[torch.Tensor] = None

    @property
    def shape(self):
        return self.s.shape

    def rows(self) -> int:
        return self.s.numel() // self.s.shape[-1]

    def fusable(self) -> bool:
        return self.s.is_cuda and self._y is None

    def materialize(self) -> torch.Tensor:
        if self._y is None:
            from . import rmsnorm

            self._y = rmsnorm(self.s, self.w, self.eps)
        return self._y

    @staticmethod
    def force(x):
        """A tensor for anything that is not a GEMV consumer."""
        return x.materialize() if isinstance(x, LazyNorm) else x


def is_q(w) -> bool:
    """An fp8 projection weight (models/llama.py QTensor: e4m3 bytes ``q`` [N, K] + per-row scales ``s``)."""
    return not isinstance(w, torch.Tensor) and hasattr(w, "q") and hasattr(w, "s")


def gemv_q_ok(m: int, n: int, k: int) -> bool:
    """Shapes of the W8A16 decode GEMV (gemv.hip WQ: fp8 weights, bf16 activations): up to 4 rows (the fused
    norm / RoPE / residual epilogues: 2), whole 1 KiB weight chunks."""
    return m <= 4 and k % 1024 == 0 and n % 16 == 0


# W4A16 decode: a Q4Tensor (models/llama.py: OCP MXFP4 q / e plus the dequantised bf16 copy w) takes the fp4 GEMV
# (gemv.hip W4) at its shapes and everything else runs the bf16 kernels on ``.w`` — the same product.  Env
# CHRONOS_W4A16_DECODE=0 (or this flag) forces ``.w`` everywhere: the A/B switch, and what the tests compare against
# (a packed-only Q4Tensor has no ``.w``: there ``w4_dense`` expands it into the model's scratch, so the switch means
# "expand everywhere" and gives copy mode's bits).
# Above the GEMV's M, up to 64 rows, a Q4Tensor call takes the W4A16 mode of the skinny MFMA GEMM where ``w4_plan``
# has a measured row for its shape (W4_SKINNY above), and at 65-512 rows the mid-M W4A16 GEMM where ``w4m_plan`` has
# one (W4_MID above).  The flag forces the copy / the expansion there too.
_W4A16_DECODE = os.environ.get("CHRONOS_W4A16_DECODE", "1") != "0"
# Largest M routed to the fp4 kernel (env CHRONOS_W4_MAX_M; the kernel takes up to 4).  Only what wins is routed:
# on cold 8B weights the fp4 GEMV beats the bf16 GEMV on ``.w`` 1.30-1.75x at M = 1 on all four projections, and at
# M = 2 and M = 4 it loses on all four, to the bf16 GEMV (0.57-0.90x) and more so to the skinny MFMA GEMM that ``.w``
# is routed to there (0.29-0.79x) — scripts/bench_gemv_w4.py, profiles/mxfp4/gemv_table.jsonl.  So the GEMV keeps M = 1
# only (the tests raise this to reach its M = 2..4 instantiations); two-stream decode and jump-forward chunks go to the
# W4A16 mode of the skinny MFMA GEMM instead (``w4_plan``), which does beat the routed bf16 kernel there.
W4_MAX_M = int(os.environ.get("CHRONOS_W4_MAX_M", "1"))
# fp4 GEMV / W4A16 skinny GEMM launches issued from Python (captured graphs replay them uncounted)
w4_stats = {"gemv_launches": 0, "skinny_launches": 0, "expand_launches": 0, "mid_launches": 0}


# W8A16 skinny GEMM launches issued from Python (captured graphs replay them uncounted)
w8_stats = {"skinny_launches": 0}


def is_w4(w) -> bool:
    """An MXFP4 projection weight (models/llama.py Q4Tensor: packed e2m1 ``q``, e8m0 ``e``, bf16 copy ``w`` — None in
    the packed-only mode)."""
    return not isinstance(w, torch.Tensor) and hasattr(w, "q") and hasattr(w, "e") and hasattr(w, "w")


class W4Scratch:
    """The packed-only MXFP4 model's one bf16 expansion buffer (``LlamaWeights.scratch``), sized to its largest
    projection.  Every ``w4_dense`` call overwrites it, so its contents live from one expansion to the GEMM issued
    right after it and reuse is safe under stream order only: ``acquire`` remembers the stream of the last use and,
    when the next use comes on another stream, makes that stream wait for everything issued so far on the previous one
    (the previous GEMM included).  The model issues every projection on the current stream — the TP overlap paths put
    only the all-reduces on a side stream — so in practice the wait never fires.  Entering or leaving a graph capture
    changes the stream too, but both sides of that boundary are ordered by the capture itself (it begins after the
    device is idle and a replay is one launch on the stream that issues it), and an event wait across it would be an
    illegal cross-capture dependency: no wait there."""

    def __init__(self, numel: int, device):
        self.buf = torch.empty(int(numel), dtype=torch.bfloat16, device=device)
        self._stream = None
        self._capturing = False

    def acquire(self) -> torch.Tensor:
        cur = torch.cuda.current_stream(self.buf.device)
        capturing = torch.cuda.is_current_stream_capturing()
        if self._stream is not None and cur != self._stream and capturing == self._capturing:
            cur.wait_stream(self._stream)
        self._stream, self._capturing = cur, capturing
        return self.buf


def w4_expand(q: torch.Tensor, e: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [N, K] of MXFP4 q [N, K / 2] / e [N, K / 32], bit-equal to ``reference.dequantize_mxfp4``: one launch of
    csrc/kernels/w4_expand.hip into ``out`` (any contiguous bf16 buffer of >= N K elements, 16-B aligned; its first N K
    elements are returned as the matrix) or into a new tensor.  CPU tensors take the reference."""
    n, k = q.shape[0], q.shape[1] * 2
    if not q.is_cuda:
        from . import reference

        w = reference.dequantize_mxfp4(q, e)
        if out is None:
            return w
        dst = out.view(-1)[:n * k].view(n, k)
        dst.copy_(w)
        return dst
    from . import _k

    if out is None:
        out = torch.empty(n, k, dtype=torch.bfloat16, device=q.device)
    _k().w4_expand(q, e, out)
    return out.view(-1)[:n * k].view(n, k)


def w4_dense(w) -> torch.Tensor:
    """The bf16 [N, K] form of a Q4Tensor for a bf16 kernel: the resident copy where there is one (no launch, as
    before), else the model's scratch after one expansion launch on the current stream — valid until the next
    ``w4_dense`` call, so the caller's GEMM goes out right after it.  CPU: the reference dequantisation."""
    if w.w is not None:
        return w.w
    if not w.q.is_cuda:
        from . import reference

        return reference.dequantize_mxfp4(w.q, w.e)
    if w.scratch is None:
        raise RuntimeError("packed-only Q4Tensor without an expansion scratch (LlamaWeights.attach_scratch)")
    w4_stats["expand_launches"] += 1
    return w4_expand(w.q, w.e, w.scratch.acquire())


def gemv_w4_ok(m: int, n: int, k: int) -> bool:
    """Shapes of the W4A16 decode GEMV (gemv.hip W4: mxfp4 weights, bf16 activations): up to 4 rows (the fused
    norm / RoPE / residual epilogues: 2), whole 1024-element chunks (32 MX blocks), 16 rows per group."""
    return 1 <= m <= 4 and k % 1024 == 0 and n % 16 == 0


def _w4_route(t: torch.Tensor, m: int, n: int, k: int, mmax: int = 4) -> bool:
    """True: the fp4 GEMV takes this call (the caller launches it and counts it in ``w4_stats``); False: the caller
    goes on down the ladder."""
    return bool(_W4A16_DECODE and t.is_cuda and m <= min(mmax, W4_MAX_M) and gemv_w4_ok(m, n, k))


def decode_gemv_weight(t: torch.Tensor, w, m: int, n: int, k: int):
    """What a fused decode GEMV epilogue (``ops.qkv_rope``, M <= 2) streams for this projection weight: (weight, fp8 row
    scales or None, mxfp4 block scales or None), or None off the GEMV's shapes.  A Q4Tensor off the fp4 GEMV's shapes
    goes in as ``w4_dense`` — asked only once the bf16 GEMV takes the call: no expansion for a call that is not made."""
    if is_w4(w):
        if _w4_route(t, m, n, k, 2):
            return w.q, None, w.e
        return (w4_dense(w), None, None) if t.is_cuda and m <= 2 and gemv_ok(m, n, k) else None
    if not (t.is_cuda and m <= 2):
        return None
    if is_q(w):
        return (w.q, w.s, None) if gemv_q_ok(m, n, k) else None
    return (w, None, None) if gemv_ok(m, n, k) else None


def _w4_gemm(x, w, mode: int, m: int, n: int, k: int, fuse: bool, resid=None):
    """The W4A16 MFMA launch for a Q4Tensor call the GEMV did not take — the skinny kernel up to W4_SKINNY_MAX_M rows,
    the mid-M GEMM (gemm_w4m.hip) above: (y, partials), or None when ``w4_plan`` / ``w4m_plan`` has no route (the
    caller substitutes ``w4_dense``).  ``fuse``: x is a fusable LazyNorm and goes in as the kernel's NORMP prologue."""
    mid = m > W4_SKINNY_MAX_M
    plan = (w4m_plan if mid else w4_plan)(m, n, k, mode, w.w is None)
    if plan is None:
        return None
    from . import _k

    w4_stats["mid_launches" if mid else "skinny_launches"] += 1
    t, resid, part, eps = (x.s, None, x.part, x.eps) if fuse else (LazyNorm.force(x), resid, None, 1e-5)
    if mid:
        return _k().gemm_w4m(t.reshape(-1, k), w.q, w.e, mode, plan[0], plan[1], resid, part, eps)
    return _k().gemm_skinny(t.reshape(-1, k), w.q, mode, plan[0], plan[1], resid, part, eps, w.e)


def _w8_gemm(x, w, mode: int, m: int, n: int, k: int, fuse: bool, resid=None):
    """The W8A16 skinny launch for an ``a16`` QTensor call the GEMV did not take: (y, partials), or None when
    ``w8_plan`` has no route (the caller runs the W8A8 op).  ``fuse``: x is a fusable LazyNorm and goes in as the
    kernel's NORMP prologue."""
    plan = w8_plan(m, n, k, mode)
    if plan is None:
        return None
    from . import _k

    w8_stats["skinny_launches"] += 1
    t, resid, part, eps = (x.s, None, x.part, x.eps) if fuse else (LazyNorm.force(x), resid, None, 1e-5)
    return _k().gemm_skinny(t.reshape(-1, k), w.q, mode, plan[0], plan[1], resid, part, eps, None, w.s)


def _q_fallback(x, w, swiglu: bool = False) -> torch.Tensor:
    """fp8 weight off the W8A16 GEMV shapes: quantise the activations and run the W8A8 op."""
    from . import qlinear, quant_rows

    xq, xs = quant_rows(LazyNorm.force(x).reshape(-1, w.shape[1]))
    y = qlinear(xq, xs, w.q, w.s, swiglu)
    return y.view(*x.shape[:-1], y.shape[-1])


def _gemv_resid(x, w: torch.Tensor, resid: torch.Tensor, ws=None, we=None) -> ResidOut:
    """The decode GEMV's residual producer (gemv.hip kResid) on bf16 weights, fp8 bytes (``ws``) or mxfp4 (``we``)."""
    from . import _k

    s = torch.empty(resid.shape, dtype=resid.dtype, device=resid.device)
    return ResidOut(s, _k().gemv_resid(x.reshape(-1, x.shape[-1]), w, resid, s, ws, we))


def gemv_resid(x: torch.Tensor, w: torch.Tensor, resid: torch.Tensor, a16: bool = False) -> ResidOut:
    """Producer (O / down projection, TP=1): the new residual stream s = bf16(bf16(x @ w.T) + resid) and the RMSNorm
    partial sums of s^2, in one launch — the GEMV at M <= GEMV_MAX_M, the batched GEMM's kResid epilogue above.  ``w``
    may be an fp8 QTensor at the W8A16 GEMV shapes (resid_ok(..., fp8=True)), or with ``a16`` wherever ``resid_ok_a16``
    says so (the W8A16 skinny kernel's kResid epilogue above the GEMV's rows).  Only where the predicate says so."""
    return _project(x, w, PP_RESID, resid, a16=a16)


def resid_ok(m: int, n: int, k: int, fp8: bool = False) -> bool:
    """Shapes of the residual-epilogue producer: the M <= 2 GEMV shapes (gemv.hip kResid) and the batched GEMM's
    (gemm_pp.hip kResid) where the plan takes it; fp8 weights: the W8A16 GEMV shapes only.  An mxfp4 Q4Tensor asks
    as bf16 (fp8=False): ``gemv_resid`` runs its fp4 producer where that takes the shape and the bf16 one on ``.w``
    otherwise, so whatever is true for bf16 is true for it."""
    if fp8:
        return m <= min(GEMV_MAX_M, 2) and gemv_q_ok(m, n, k)
    if m <= GEMV_MAX_M:
        return m <= 2 and gemv_ok(m, n, k)  # (the GEMV's residual epilogue: M <= 2)
    return pp_plan(m, n, k, PP_RESID) is not None


def resid_ok_a16(m: int, n: int, k: int) -> bool:
    """The residual-epilogue producer of an fp8 QTensor for an ``a16`` caller: the W8A16 GEMV shapes, as
    ``resid_ok(..., fp8=True)``, and above two rows the W8A16 skinny kernel's kResid route where ``w8_plan`` has one."""
    return resid_ok(m, n, k, True) or (m > 2 and w8_plan(m, n, k, PP_RESID) is not None)


def w8a16_step_ok(T: int, shapes) -> bool:
    """True when every projection of a layer has a W8A16 route at T rows — ``shapes``: (N, K, epilogue) of QKV, O,
    gate_up and down — so that a W8A16 step above the GEMV's rows never pays ``_q_fallback``'s quantisation launch:
    at T <= 2 the W8A16 GEMV's shapes, above that the skinny kernel's route (``w8_plan``) for each of them."""
    for n, k, mode in shapes:
        if T <= 2:
            ok = resid_ok(T, n, k, True) if mode == PP_RESID else gemv_q_ok(T, n, k)
        else:
            ok = w8_plan(T, n, k, mode) is not None
        if not ok:
            return False
    return True


def gemv_ok(m: int, n: int, k: int, swiglu: bool = False) -> bool:
    """Shapes routed to the hand-written decode GEMV (csrc/kernels/gemv.hip): K % 512, N % 16, M <= GEMV_MAX_M (1 by
    default; M = 2 only below LM-head widths when raised)."""
    if k % 512 or n % 16:
        return False
    return m == 1 or (m <= GEMV_MAX_M and n <= 32768)


def mfma_swiglu_ok(m: int, n: int, k: int) -> bool:
    """Fused gate_up + SwiGLU on the MFMA GEMM: the measured winning range (3 <= M <= 128)."""
    return 3 <= m <= 128 and k % 64 == 0 and n % 128 == 0


def _gemv(x, w: torch.Tensor, swiglu: bool = False, ws=None, we=None, fuse: bool = False) -> torch.Tensor:
    """The decode GEMV on bf16 weights, fp8 bytes (``ws``: row scales) or mxfp4 (``we``: block scales).  ``fuse``: x is
    a fusable LazyNorm and its norm the kernel's per-row output scale (gemv.hip NORMP); otherwise x is materialised."""
    from . import _k

    if fuse:
        return _k().gemv_normp(x.s, x.part, x.eps, w, swiglu, ws, we)
    x = LazyNorm.force(x)
    y = _k().gemv(x.reshape(-1, x.shape[-1]), w, swiglu, ws, we)
    return y.view(*x.shape[:-1], y.shape[-1])


def mfma_gemm(x: torch.Tensor, w: torch.Tensor, swiglu: bool = False, stages: int = 3) -> torch.Tensor:
    from . import _k

    k = x.shape[-1]
    y = _k().gemm(x.reshape(-1, k), w, swiglu, stages)
    return y.view(*x.shape[:-1], y.shape[-1])


def _project(x, w, mode: int, resid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
             a16: bool = False):
    """The one dispatcher behind ``linear`` (PP_PLAIN), ``gate_up_silu`` (PP_SWIGLU) and ``gemv_resid`` (PP_RESID, with
    ``resid``): the ladder of the module docstring, walked once.  ``out`` (linear only) keeps the call off every
    Q4Tensor kernel, every fused norm and every planned GEMM: it is the library's ``out=``.  (The plain decode GEMV and
    the fp8 paths do not look at it and return a new tensor, as they always did.)  ``a16``: an fp8 QTensor call the
    W8A16 GEMV does not take may go to the W8A16 skinny kernel (``w8_plan``); it changes nothing for other weights."""
    lazy = isinstance(x, LazyNorm)
    t = x.s if lazy else x
    k = t.shape[-1]
    m, n = t.numel() // k, w.shape[0]
    swiglu = mode == PP_SWIGLU
    fuse = lazy and x.fusable() and mode != PP_RESID  # the folded norm can go in as the kernel's prologue

    def shaped(y, part=None):
        return ResidOut(y.view(resid.shape), part) if mode == PP_RESID else y.view(*t.shape[:-1], y.shape[-1])

    if is_w4(w):  # mxfp4 weights: a W4A16 kernel where one is routed, else the bf16 steps on the dense form
        if t.is_cuda and out is None:
            # the fp4 residual producer at the W8A16 precedent's rows (M <= min(GEMV_MAX_M, 2)); 8 rows per group: N / 8
            # partials, which the consumer reads as float4
            cap, nmul = (min(GEMV_MAX_M, 2), 32) if mode == PP_RESID else (4, 16)
            if n % nmul == 0 and _w4_route(t, m, n, k, cap):
                w4_stats["gemv_launches"] += 1
                if mode == PP_RESID:
                    return _gemv_resid(x, w.q, resid, None, w.e)
                return _gemv(x, w.q, swiglu, None, w.e, fuse and m <= 2)
            hit = _w4_gemm(x, w, mode, m, n, k, fuse, resid.reshape(m, -1) if mode == PP_RESID else None)
            if hit is not None:
                return shaped(*hit)
        w = w4_dense(w)
    if is_q(w):  # fp8 weights: the W8A16 GEMV (folded norm fused at M <= 2 when x is a LazyNorm), else W8A8
        # a16: the GEMV keeps its fused-epilogue rows (M <= 2); above them the skinny kernel where it has a route — at
        # M = 3-4 too, where the GEMV is the slower of the two (models/llama.py _W8A16_DECODE)
        gemv = gemv_q_ok(m, n, k)
        if a16 and t.is_cuda and not (gemv and m <= 2):
            hit = _w8_gemm(x, w, mode, m, n, k, fuse, resid.reshape(m, -1) if mode == PP_RESID else None)
            if hit is not None:
                return shaped(*hit)
        if mode == PP_RESID:
            return _gemv_resid(x, w.q, resid, w.s)
        if t.is_cuda and gemv:
            return _gemv(x, w.q, swiglu, w.s, None, fuse and m <= 2)
        return _q_fallback(LazyNorm.force(x), w, swiglu)
    if mode == PP_RESID:
        if m > GEMV_MAX_M:
            return shaped(*pp_gemm(x, w, PP_RESID, pp_plan(m, n, k, PP_RESID), resid.reshape(m, -1)))
        return _gemv_resid(x, w, resid)
    if t.is_cuda:
        if gemv_ok(m, n, k, swiglu):
            return _gemv(x, w, swiglu, fuse=fuse and out is None)
        plan = pp_plan(m, n, k, mode) if out is None else None
        if plan is not None:
            if fuse:
                y, _ = pp_gemm(x.s, w, mode, plan, None, x.part, x.eps)
            else:
                y, _ = pp_gemm(LazyNorm.force(x), w, mode, plan)
            return shaped(y)
    x = LazyNorm.force(x)
    if swiglu:
        if x.is_cuda and mfma_swiglu_ok(m, n, k):
            return mfma_gemm(x, w, True)
        from . import silu_mul

        return silu_mul(_project(x, w, PP_PLAIN))
    if out is not None:
        return torch.matmul(x, w.t(), out=out)
    return torch.matmul(x, w.t())


def gate_up_silu(x: torch.Tensor, w_gu: torch.Tensor, a16: bool = False) -> torch.Tensor:
    """silu(x @ gate.T) * (x @ up.T) with w_gu = [gate; up]: one fused launch (GEMV at M <= GEMV_MAX_M, the batched
    GEMM's SwiGLU epilogue above, with the folded input norm when x is a LazyNorm), else GEMM + silu_mul."""
    return _project(x, w_gu, PP_SWIGLU, a16=a16)


def linear(x, w: torch.Tensor, out: Optional[torch.Tensor] = None, a16: bool = False) -> torch.Tensor:
    return _project(x, w, PP_PLAIN, out=out, a16=a16)
