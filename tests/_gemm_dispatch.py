"""Launch-log characterisation of the projection GEMM dispatch (ops/gemm.py, ops.qkv_rope), on the CPU.

The routing is pure Python but only reaches the hand-written kernels for tensors whose ``is_cuda`` is true.  Here the
operands are zero-stride CPU tensors of a subclass that says it is on the device, ``chronos.ops._k`` returns a recorder
whose every op appends its call to a log and returns empty tensors of the right shapes, and ``torch.matmul`` /
``torch._scaled_mm`` are replaced by loggers, so the extension is never loaded and nothing is computed.  A logged call
holds the op name, every scalar argument (mode / swiglu flag, cfg, split-K, eps) and, for every tensor argument, WHICH
operand it is — found by storage identity, never by shape: ``w`` (bf16), ``w.w`` (the resident copy of a Q4Tensor),
``scratch``, ``q`` / ``e``, ``q8`` / ``ws`` (fp8), ``x``, ``s`` / ``part`` (the raw stream of a LazyNorm), ``y``
(its materialised form), ``@op`` (what an earlier logged op returned) — with None for an absent optional argument.

Routing is piecewise constant in M, so a case — (entry point, shape, weights, x, switches) — is stored as a run-length
list of [first M, last M, index into "logs"] in tests/golden/gemm_dispatch.json; ``python tests/_gemm_dispatch.py
--write PATH`` regenerates the file, ``--time`` prints the dispatch cost per call.  Only the public surface is used
(the entry points, LazyNorm, Q4Tensor, QTensor and the module switches), so the same file runs on any revision.
"""
from __future__ import annotations

import contextlib
import json
import os
import sys
import time

import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chronos import ops  # noqa: E402
from chronos.models.llama import Q4Tensor, QTensor  # noqa: E402
from chronos.ops import gemm  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_dispatch.json")
PLAN = os.path.join(os.path.dirname(os.path.abspath(gemm.__file__)), "gemm_plan.json")
MS = list(range(1, 601)) + [768, 1000, 1024, 2048, 4096, 16384, 20000]
SMALL = ((1536, 1024, 0), (1024, 1024, 2), (5632, 1024, 1), (1024, 2816, 2))
# shapes the kernels refuse: N % 16 (and % 4), K % 64, swiglu N % 128
REFUSED = ((6152, 4096, 0), (6146, 4096, 0), (4104, 4096, 2), (6144, 4128, 0), (4096, 4128, 2), (28736, 4096, 1))
SHAPES_8B = ((6144, 4096, 0), (4096, 4096, 2), (28672, 4096, 1), (4096, 14336, 2))
WEIGHTS = ("bf16", "fp8", "w4", "w4p")
XKINDS = ("plain", "lazy", "mat")
SWITCHES = (("PP_MODE", "own"), ("PP_MODE", "lib"), ("W4_SKINNY", "off"), ("W4_SKINNY", "model"), ("W4_MID", "off"),
            ("W4_MID", "model"), ("_W4A16_DECODE", False), ("GEMV_MAX_M", 2), ("W4_MAX_M", 4))
# the switch-hygiene case: assigned in the middle of a sweep (M range -> switch, value), then assigned back, with no
# cache touched by hand: a switch takes effect at once
HYGIENE = ((20, 30, "W4_SKINNY", "off"), (40, 50, "W4_SKINNY", "model"), (70, 80, "W4_MID", "off"),
           (100, 120, "W4_MID", "model"))
# the switch variants are thinned, not the default grid: every M up to 140, then the plan rows with both neighbours;
# and a switch that only Q4Tensor routing reads runs on the Q4Tensor weights alone
MS_SWITCH = list(range(1, 141)) + [191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512, 513, 600] + MS[600:]
W4_ONLY = ("W4_SKINNY", "W4_MID", "_W4A16_DECODE", "W4_MAX_M")


def plan_shapes() -> list[tuple[int, int, int]]:
    with open(PLAN) as fh:
        raw = json.load(fh)
    keys = []
    for sec in ("plans", "qplans", "w4plans", "w4mplans"):
        for k in raw.get(sec, {}):
            t = tuple(int(v) for v in k.split(","))
            if t not in keys:
                keys.append(t)
    return keys


_PLAIN = torch._C.DisableTorchFunctionSubclass


class _Dev(torch.Tensor):
    """A CPU tensor that says it is on the device (reshape and view keep the subclass)."""

    @property
    def is_cuda(self):
        return True

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):  # the default's behaviour, without its generality
        with _PLAIN():
            out = func(*args, **(kwargs or {}))
        return out.as_subclass(cls) if type(out) is torch.Tensor else out


def dev(shape, dtype=torch.bfloat16) -> torch.Tensor:
    """No memory behind it: one element, every stride 0."""
    with _PLAIN():
        return torch.empty(1, dtype=dtype).expand(tuple(int(v) for v in shape)).as_subclass(_Dev)


def _sid(t: torch.Tensor) -> int:
    return t.untyped_storage().data_ptr()


class Recorder:
    """Stands in for ``torch.ops.chronos``: logs, computes nothing."""

    def __init__(self):
        self.names: dict[int, str] = {}  # storage -> operand name
        self.operands: dict = {}
        self.log: list = []

    def operand(self, name: str, shape, dtype=torch.bfloat16) -> torch.Tensor:
        """The named operand of that shape: made once and kept, so that no storage address is ever reused."""
        key = (name, tuple(shape), dtype)
        t = self.operands.get(key)
        if t is None:
            t = self.operands[key] = dev(shape, dtype)
            self.names[_sid(t)] = name
        return t

    def begin(self) -> None:
        self.log = []

    def _arg(self, a):
        if isinstance(a, torch.Tensor):
            s = _sid(a)
            return self.names.get(s) or "?" + str(a.dtype)
        if isinstance(a, float):
            return float(f"{a:.6g}")
        return a

    def _out(self, op: str, shape, dtype=torch.bfloat16) -> torch.Tensor:
        return self.operand("@" + op, shape, dtype)  # (made once per shape like the operands: the name is what counts)

    def record(self, op: str, args, kwargs=None) -> None:
        with _PLAIN():
            self._record(op, args, kwargs)

    def _record(self, op: str, args, kwargs) -> None:
        row = [op] + [self._arg(a) for a in args]
        while row[-1] is None:
            row.pop()
        for k in sorted(kwargs or {}):
            row.append([k, self._arg(kwargs[k])])
        self.log.append(row)

    def _y(self, op, x, w, half):
        n = w.shape[0]
        return self._out(op, (x.numel() // x.shape[-1], n // 2 if half else n))

    def _gemm3(self, op, x, w, mode):
        m = x.numel() // x.shape[-1]
        part = self._out(op + ".part", (m, 1), torch.float32) if mode == 2 else self._out("none", (0,))
        return self._y(op, x, w, mode == 1), part

    # what each op returns: empty tensors of the right shapes
    RETURNS = {
        "gemm_pp": lambda r, x, w, mode, *a: r._gemm3("gemm_pp", x, w, mode),
        "gemm_skinny": lambda r, x, w, mode, *a: r._gemm3("gemm_skinny", x, w, mode),
        "gemm_w4m": lambda r, x, q, e, mode, *a: r._gemm3("gemm_w4m", x, q, mode),
        "gemv": lambda r, x, w, swiglu, *a: r._y("gemv", x, w, swiglu),
        "gemm": lambda r, x, w, swiglu, *a: r._y("gemm", x, w, swiglu),
        "gemv_normp": lambda r, s, part, eps, w, swiglu, *a: r._out(
            "gemv_normp", (*s.shape[:-1], w.shape[0] // 2 if swiglu else w.shape[0])),
        "gemv_resid": lambda r, x, w, *a: r._out("gemv_resid", (x.shape[0], w.shape[0] // 8), torch.float32),
        "w4_expand": lambda r, *a: None,
        "qkv_rope": lambda r, *a: None,
        "rmsnorm": lambda r, x, *a: r._out("rmsnorm", x.shape),
        "silu_mul": lambda r, gu: r._out("silu_mul", (*gu.shape[:-1], gu.shape[-1] // 2)),
        "quant_rows": lambda r, x, *a: (r._out("quant_rows.q", x.shape, torch.uint8),
                                        r._out("quant_rows.s", x.shape[:-1], torch.float32)),
        "qlinear": lambda r, xq, xs, wq, ws, swiglu, *a: r._y("qlinear", xq, wq, swiglu),
        "qgemm_lg": lambda r, xq, xs, wq, ws, swiglu, *a: r._y("qgemm_lg", xq, wq, swiglu),
    }

    def __getattr__(self, op):
        ret = Recorder.RETURNS.get(op)
        if ret is None:
            raise AttributeError(f"recorder: no op {op!r}")

        def call(*args, **kwargs):
            self.record(op, args, kwargs)
            with _PLAIN():
                return ret(self, *args)

        self.__dict__[op] = call
        return call


class _Scratch:
    def __init__(self, buf):
        self.buf = buf

    def acquire(self):
        return self.buf


@contextlib.contextmanager
def harness():
    """The recorder in place of the extension and of the library GEMMs; everything restored afterwards."""
    rec = Recorder()
    old = (ops._k, torch.matmul, torch._scaled_mm)

    def matmul(a, b, out=None):
        rec.record("matmul", (a, b), {"out": out} if out is not None else None)
        return rec._out("matmul", (*a.shape[:-1], b.shape[-1]))

    def scaled_mm(a, b, **kw):
        rec.record("scaled_mm", (a, b))
        return rec._out("scaled_mm", (a.shape[0], b.shape[-1]))

    ops._k, torch.matmul, torch._scaled_mm = (lambda: rec), matmul, scaled_mm
    try:
        yield rec
    finally:
        ops._k, torch.matmul, torch._scaled_mm = old


def make_weight(rec: Recorder, kind: str, n: int, k: int):
    if kind == "bf16":
        return rec.operand("w", (n, k))
    if kind == "fp8":
        return QTensor(rec.operand("q8", (n, k), torch.uint8), rec.operand("ws", (n,), torch.float32))
    q, e = rec.operand("q", (n, k // 2), torch.uint8), rec.operand("e", (n, k // 32), torch.uint8)
    if kind == "w4":
        return Q4Tensor(q, e, rec.operand("w.w", (n, k)))
    return Q4Tensor(q, e, None, _Scratch(rec.operand("scratch", (n * k,))))


def make_x(rec: Recorder, kind: str, m: int, k: int):
    if kind == "plain":
        return rec.operand("x", (m, k))
    s, part = rec.operand("s", (m, k)), rec.operand("part", (m, 8), torch.float32)
    y = rec.operand("y", (m, k)) if kind == "mat" else None
    return ops.LazyNorm(s, part, rec.operand("normw", (k,)), 1e-6, y)


ENTRIES = {0: ("linear", "linear_out", "qkv_rope"), 1: ("gate_up_silu",), 2: ("gemv_resid", "linear")}


def run_one(rec: Recorder, entry: str, w, xkind: str, m: int, n: int, k: int) -> dict:
    """One call of one entry point; the log of the case."""
    rec.begin()
    x = make_x(rec, xkind, m, k)
    before = dict(gemm.w4_stats)
    res: dict = {}
    try:
        if entry == "linear":
            ops.linear(x, w)
        elif entry == "linear_out":
            ops.linear(x, w, out=rec.operand("out", (m, n)))
        elif entry == "gate_up_silu":
            ops.gate_up_silu(x, w)
        elif entry == "gemv_resid":  # as models/llama.py _out_proj asks: resid_ok first, ops.linear otherwise
            res["resid_ok"] = bool(ops.resid_ok(m, w.shape[0], w.shape[1], ops.is_q(w)))
            if res["resid_ok"]:
                out = ops.gemv_resid(x, w, rec.operand("resid", (m, n)))
                res["ret"] = [rec._arg(out.s), rec._arg(out.part)]
        elif entry == "qkv_rope":
            t = [rec.operand(nm, (4,), torch.int32) for nm in ("pos", "tok_seq", "block_table")]
            t += [rec.operand(nm, (4,)) for nm in ("cos_sin", "q_out", "k_cache", "v_cache")]
            res["ret"] = bool(ops.qkv_rope(x, w, *t, 32, 8, 1.0, 1.0))
    except Exception as exc:  # noqa: BLE001 - a raise is part of the behaviour
        res["raised"] = type(exc).__name__
    res["calls"] = rec.log
    delta = {key: gemm.w4_stats[key] - before[key] for key in before if gemm.w4_stats[key] != before[key]}
    if delta:
        res["stats"] = delta
    return res


def _entry_ms(entry: str, ms) -> list[int]:
    return [1, 2, 3, 4] if entry == "qkv_rope" else ms


def _xkinds(entry: str):
    return ("plain",) if entry == "gemv_resid" else XKINDS  # the producer's x is a plain tensor (llama.py _out_proj)


class Sweep:
    def __init__(self):
        self.logs: list[str] = []
        self.index: dict[str, int] = {}
        self.cases: dict[str, list] = {}

    def intern(self, log: dict) -> int:
        key = json.dumps(log, sort_keys=True, separators=(",", ":"))
        if key not in self.index:
            self.index[key] = len(self.logs)
            self.logs.append(key)
        return self.index[key]

    def add(self, case: str, m: int, log: dict) -> None:
        i = self.intern(log)
        runs = self.cases.setdefault(case, [])
        if runs and runs[-1][2] == i:
            runs[-1][1] = m
        else:
            runs.append([m, m, i])

    def result(self) -> dict:
        return {"logs": [json.loads(s) for s in self.logs], "cases": self.cases}


def _clear_cache() -> None:
    cache = getattr(gemm, "_plan_cache", None)  # the switch variants, as the routing tests do around a switch
    if cache is not None:
        cache.clear()


def sweep_shapes(rec: Recorder, out: Sweep, shapes, tag: str, hygiene=(), ms=MS, weights=WEIGHTS) -> None:
    for n, k, mode in shapes:
        for wkind in weights:
            w = make_weight(rec, wkind, n, k)
            for entry in ENTRIES[mode]:
                for xkind in _xkinds(entry):
                    case = f"{entry}|{n},{k},{mode}|{wkind}|{xkind}|{tag}"
                    for m in _entry_ms(entry, ms):
                        for lo, hi, name, val in hygiene:
                            if m == lo:
                                setattr(gemm, name, val)
                            elif m == hi + 1:
                                setattr(gemm, name, "plan")
                        out.add(case, m, run_one(rec, entry, w, xkind, m, n, k))


def collect() -> dict:
    """The whole grid: {"logs": [...], "cases": {case: [[first M, last M, log index], ...]}}."""
    names = sorted({name for name, _ in SWITCHES})
    saved = {name: getattr(gemm, name) for name in names}
    out = Sweep()
    shapes = plan_shapes()
    shapes += [s for s in SMALL + REFUSED if s not in shapes]
    try:
        with harness() as rec:
            sweep_shapes(rec, out, shapes, "default")
            sweep_shapes(rec, out, SHAPES_8B, "hygiene", HYGIENE, MS_SWITCH, ("w4", "w4p"))
            for name, val in SWITCHES:
                _clear_cache()
                setattr(gemm, name, val)
                try:
                    sweep_shapes(rec, out, SHAPES_8B, f"{name}={val}", (), MS_SWITCH,
                                 ("w4", "w4p") if name in W4_ONLY else WEIGHTS)
                finally:
                    setattr(gemm, name, saved[name])
                    _clear_cache()
    finally:
        for name in names:
            setattr(gemm, name, saved[name])
    return out.result()


def dumps(result: dict) -> str:
    lines = ["{", ' "logs": [']
    lines += ["  " + json.dumps(lg, sort_keys=True, separators=(",", ":")) + ("," if i + 1 < len(result["logs"]) else "")
              for i, lg in enumerate(result["logs"])]
    lines += [" ],", ' "cases": {']
    items = list(result["cases"].items())
    lines += [f"  {json.dumps(c)}: {json.dumps(runs, separators=(',', ':'))}" + ("," if i + 1 < len(items) else "")
              for i, (c, runs) in enumerate(items)]
    lines += [" }", "}"]
    return "\n".join(lines) + "\n"


def time_dispatch(repeats: int = 5) -> dict:
    """Microseconds per call of each entry point over the default grid (recorder cost included, equal on any revision)."""
    shapes = plan_shapes()
    shapes += [s for s in SMALL + REFUSED if s not in shapes]
    per: dict[str, list[float]] = {}
    with harness() as rec:
        for _ in range(repeats):
            tot: dict[str, list] = {}
            for n, k, mode in shapes:
                for wkind in WEIGHTS:
                    w = make_weight(rec, wkind, n, k)
                    for entry in ENTRIES[mode]:
                        if entry in ("qkv_rope", "linear_out"):
                            continue
                        for xkind in _xkinds(entry):
                            t0 = time.perf_counter()
                            for m in MS:
                                run_one(rec, entry, w, xkind, m, n, k)
                            acc = tot.setdefault(entry, [0.0, 0])
                            acc[0] += time.perf_counter() - t0
                            acc[1] += len(MS)
            for entry, (sec, calls) in tot.items():
                per.setdefault(entry, []).append(round(1e6 * sec / calls, 3))
    return per


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--write":
        t0 = time.perf_counter()
        text = dumps(collect())
        with open(sys.argv[2], "w") as fh:
            fh.write(text)
        print(f"{sys.argv[2]}: {len(text)} bytes in {time.perf_counter() - t0:.1f} s")
    elif len(sys.argv) == 2 and sys.argv[1] == "--time":
        print(json.dumps({"us_per_call": time_dispatch()}))
    else:
        sys.exit("usage: _gemm_dispatch.py --write PATH | --time")
