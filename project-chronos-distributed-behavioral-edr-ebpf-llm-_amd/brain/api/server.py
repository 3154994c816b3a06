"""Ollama-compatible HTTP front door of the Brain (reference README.md:57-62 `ollama serve`).

Endpoints:
  POST /api/generate   the sensor contract (chronos_sensor.py:117-120): stream=false -> one JSON object whose
                       ``response`` is the (constrained) model text; stream=true -> NDJSON chunks (Ollama default)
  POST /api/chat       Llama-3 chat template over ``messages``
  POST /api/embed      L2-normalised fp32 embeddings of ``input`` (a string or a list), pooled on the device from the
                       final-RMSNorm hidden state (protocol.py);  POST /api/embeddings  the legacy one-``prompt`` form
  GET  /api/tags, POST /api/show, GET /api/ps, GET /api/version, GET /      model listing / health (Ollama shapes)
  GET  /healthz        liveness + engine state;   GET /metrics   Prometheus text (utils/metrics.py)

Run: ``python -m chronos.brain.api --model llama3-8b --port 11434 [--dp N]`` (binds 0.0.0.0 like OLLAMA_HOST=0.0.0.0).
Backends: EngineService (one engine on this process's GPU), DPRouter (one engine process per GPU), FakeBackend
(tests / fault injection).
"""
from __future__ import annotations

import argparse
import asyncio
import json
import logging
import os
import threading
import time

from aiohttp import web

from ...utils import freeze_startup_objects
from ...utils.metrics import METRICS
from .protocol import (OLLAMA_VERSION, BadRequest, EmbedParams, GenerateParams, StopFilter, apply_stop, chat_response,
                       embed_response, stop_context_ids,
                       final_fields, generate_response, logprobs_field, now_iso, penalties_ignored)

log = logging.getLogger("chronos.api")


def make_app(backend, model_name: str = "llama3", request_timeout: float | None = None) -> web.Application:
    app = web.Application(client_max_size=64 * 2**20)
    started = time.time()

    async def _params(request, chat=False) -> GenerateParams:
        try:
            body = await request.json()
        except Exception:
            raise web.HTTPBadRequest(text=json.dumps({"error": "invalid JSON body"}), content_type="application/json")
        try:
            return GenerateParams.parse(body, chat=chat)
        except (BadRequest, ValueError, TypeError) as e:
            raise web.HTTPBadRequest(text=json.dumps({"error": str(e)}), content_type="application/json")

    async def _run(params, chat: bool, request):
        model = params.model or model_name
        if not params.stream:
            try:
                coro = backend.generate(params)
                req = await (asyncio.wait_for(coro, request_timeout) if request_timeout else coro)
            except asyncio.TimeoutError:
                return web.json_response({"error": "generation timed out"}, status=504)
            if getattr(req, "error", None):
                # a request the engine rejected is the client's fault (400); a failed engine step is ours (500)
                internal = (getattr(req, "meta", None) or {}).get("internal_error", False)
                return web.json_response({"error": req.error}, status=500 if internal else 400)
            ctx = None
            hit = False
            if params.stop:  # checked on the finished text: cut at the first stop string, reason "stop"
                req.text, hit = apply_stop(req.text, params.stop)
                if hit:
                    req.done_reason = "stop"
                    tok = getattr(backend, "tok", None)
                    if tok is not None and not chat:
                        ctx = stop_context_ids(tok, req.prompt_ids, req.out_ids, req.text)
            lps = None
            if params.logprobs >= 0:
                lps = logprobs_field(getattr(backend, "tok", None), req, req.text if hit else None)
            ignored = penalties_ignored(params, req) + (("logprobs",) if params.logprobs >= 0 and lps is None else ())
            if chat:
                body = chat_response(model, req, ignored)
            else:
                body = generate_response(model, req, ignored)
                if ctx is not None:
                    body["context"] = ctx
            if lps is not None:
                body["logprobs"] = lps
            return web.json_response(body)
        resp = web.StreamResponse(headers={"Content-Type": "application/x-ndjson"})
        await resp.prepare(request)
        sf = StopFilter(params.stop) if params.stop else None

        def piece(text: str, done: bool = False) -> dict:
            chunk = {"model": model, "created_at": now_iso()}
            if chat:
                chunk["message"] = {"role": "assistant", "content": text}
            else:
                chunk["response"] = text
            chunk["done"] = done
            return chunk

        gen = backend.generate_stream(params)
        async for text, final in gen:
            if sf is not None:
                text = sf.feed(text) if final is None else sf.flush()
                if final is not None and text:
                    await resp.write((json.dumps(piece(text)) + "\n").encode())
                    text = ""
                if final is None and sf.hit:
                    # stop string seen: emit what precedes it, end the reply, and close the generator, which
                    # cancels the engine request (its slot and KV blocks are freed at the next step)
                    if text:
                        await resp.write((json.dumps(piece(text)) + "\n").encode())
                    await gen.aclose()
                    await resp.write((json.dumps(dict(piece("", True), done_reason="stop")) + "\n").encode())
                    break
            if final is None:
                if not text:
                    continue
                chunk = piece(text)
            else:
                if getattr(final, "error", None):
                    chunk = {"error": final.error}
                else:
                    chunk = {"model": model, "created_at": now_iso()}
                    if chat:
                        chunk["message"] = {"role": "assistant", "content": ""}
                    else:
                        chunk["response"] = ""
                        chunk["context"] = [int(t) for t in list(final.prompt_ids) + list(final.out_ids)]
                    chunk.update(final_fields(final))
                    ignored = penalties_ignored(params, final)
                    if params.logprobs >= 0:  # the whole list on the final chunk (protocol.py: deviation from Ollama)
                        lps = logprobs_field(getattr(backend, "tok", None), final)
                        if lps is None:
                            ignored += ("logprobs",)
                        else:
                            chunk["logprobs"] = lps
                    if ignored:
                        chunk["ignored_options"] = list(ignored)
            await resp.write((json.dumps(chunk) + "\n").encode())
        await resp.write_eof()
        return resp

    async def generate(request):
        return await _run(await _params(request), False, request)

    async def chat(request):
        return await _run(await _params(request, chat=True), True, request)

    async def _embed(request, legacy: bool):
        def err(msg, status):
            return web.json_response({"error": msg}, status=status)

        try:
            body = await request.json()
        except Exception:
            return err("invalid JSON body", 400)
        try:
            p = EmbedParams.parse(body, legacy=legacy)
        except (BadRequest, ValueError, TypeError) as e:
            return err(str(e), 400)
        fn = getattr(backend, "embed", None)
        if fn is None:
            return err("this backend does not serve embeddings", 501)
        t0 = time.perf_counter()
        try:
            coro = fn(list(p.inputs), p.truncate, p.num_ctx or None)
            reqs = await (asyncio.wait_for(coro, request_timeout) if request_timeout else coro)
        except asyncio.TimeoutError:
            return err("embedding timed out", 504)
        for r in reqs:
            if getattr(r, "error", None):  # rejected by the engine: the client's fault; a failed step: ours
                internal = (getattr(r, "meta", None) or {}).get("internal_error", False)
                return err(r.error, 500 if internal else 400)
        return web.json_response(embed_response(p.model or model_name, reqs, t0, legacy))

    async def embed(request):
        return await _embed(request, False)

    async def embeddings(request):
        return await _embed(request, True)

    def _model_entry():
        info = backend.info() if hasattr(backend, "info") else {}
        # (packed-only MXFP4 is the same numbers as "mxfp4": one quantization level)
        quant = {"bf16": "BF16", "fp8": "FP8", "mxfp4": "MXFP4",
                 "mxfp4-packed": "MXFP4"}[getattr(backend, "weight_dtype", "bf16")]
        return {"name": f"{model_name}:latest", "model": f"{model_name}:latest", "modified_at": now_iso(),
                "size": int(info.get("params", 0)) * 2, "digest": "chronos-random-init",
                "details": {"format": "safetensors", "family": "llama", "families": ["llama"],
                            "parameter_size": f"{info.get('params', 0) / 1e9:.1f}B", "quantization_level": quant}}

    async def tags(request):
        return web.json_response({"models": [_model_entry()]})

    async def ps(request):
        e = _model_entry()
        e["expires_at"] = "2999-01-01T00:00:00Z"  # weights stay resident (no keep_alive unload, quirk X8)
        e["size_vram"] = e["size"]
        if getattr(backend, "weight_dtype", "bf16") == "mxfp4-packed" and hasattr(backend, "resident_bytes"):
            e["size_vram"] = int(backend.resident_bytes)  # what the mode is for: q / e + bf16 rest + the scratch
        return web.json_response({"models": [e]})

    async def show(request):
        info = backend.info() if hasattr(backend, "info") else {}
        return web.json_response({"modelfile": "", "parameters": "", "template": "llama3",
                                  "details": _model_entry()["details"], "model_info": info})

    async def version(request):
        return web.json_response({"version": OLLAMA_VERSION})

    async def root(request):
        return web.Response(text="Ollama is running")

    async def healthz(request):
        info = backend.info() if hasattr(backend, "info") else {}
        ok, health = backend.health() if hasattr(backend, "health") else (True, {"status": "ok"})
        return web.json_response({**health, "uptime_s": time.time() - started, **info}, status=200 if ok else 503)

    async def metrics(request):
        return web.Response(text=METRICS.render(), content_type="text/plain")

    app.add_routes([
        web.post("/api/generate", generate), web.post("/api/chat", chat), web.post("/api/embed", embed),
        web.post("/api/embeddings", embeddings), web.get("/api/tags", tags),
        web.get("/api/ps", ps), web.post("/api/show", show), web.get("/api/version", version), web.get("/", root),
        web.get("/healthz", healthz), web.get("/metrics", metrics),
    ])
    return app


# ---------------------------------------------------------------------------------------------------------------
# fake backend (contract tests, fault injection: SURVEY.md §4.2 "contract" row, §5.3)
# ---------------------------------------------------------------------------------------------------------------


class FakeBackend:
    """Answers every request with a canned verdict.  ``mode``: "ok", "stall" (sleep ``delay`` s), "raise",
    "badjson" (response text that is not JSON), "error" (engine-level error)."""

    def __init__(self, mode: str = "ok", delay: float = 0.0, verdict: dict | None = None):
        self.mode, self.delay = mode, delay
        self.verdict = verdict or {"risk_score": 8, "verdict": "MALICIOUS", "reason": "curl -> chmod -> exec dropper"}
        self.seen: list[GenerateParams] = []

    def _req(self, params):
        from types import SimpleNamespace

        now = time.perf_counter()
        text = "not json {" if self.mode == "badjson" else json.dumps(self.verdict)
        return SimpleNamespace(text=text, error="engine failure" if self.mode == "error" else None,
                               prompt_ids=[0] * max(1, len(params.prompt) // 4), out_ids=[0] * 20, done_reason="stop",
                               t_submit=now - 0.01, t_admit=now - 0.01, t_first=now - 0.005, t_done=now)

    async def generate(self, params):
        self.seen.append(params)
        if self.mode == "stall":
            await asyncio.sleep(self.delay)
        if self.mode == "raise":
            raise RuntimeError("injected fault")
        return self._req(params)

    async def generate_stream(self, params):
        req = await self.generate(params)
        for i in range(0, len(req.text), 8):
            yield req.text[i:i + 8], None
        yield "", req

    def info(self):
        return {"engines": 0, "model": "fake", "params": 0}


# ---------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="CHRONOS Brain: Ollama-compatible Llama-3 server on MI355X")
    ap.add_argument("--host", default="0.0.0.0")
    ap.add_argument("--port", type=int, default=11434)
    ap.add_argument("--model", default="llama3-8b", help="preset (random-init) when --checkpoint is not given")
    ap.add_argument("--checkpoint", default=None, help="HF or Meta Llama-3 checkpoint directory")
    ap.add_argument("--tokenizer", default=None)
    ap.add_argument("--served-name", default="llama3")
    ap.add_argument("--dp", type=int, default=1, help="engine replicas, one process per GPU")
    ap.add_argument("--tp", type=int, default=1,
                    help="tensor-parallel degree (launch with torchrun --nproc-per-node TP: rank 0 serves HTTP, the "
                         "other ranks follow the lockstep scheduler)")
    ap.add_argument("--sequence-parallel", action="store_true", help="with --tp: sequence-parallel prefill")
    ap.add_argument("--cp", type=int, default=1,
                    help="context-parallel degree for long kill-chain prefill (torchrun launch, full weights per rank)")
    ap.add_argument("--max-slots", type=int, default=512)
    ap.add_argument("--max-model-len", type=int, default=4096)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--fake", choices=["ok", "stall", "raise", "badjson"], default=None)
    ap.add_argument("--jsonl", default=None, help="append per-request records here")
    ap.add_argument("--request-timeout", type=float, default=0.0,
                    help="seconds; a slower generation answers 504 and is cancelled in the engine (0 = none)")
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--weights", choices=["bf16", "fp8", "mxfp4", "mxfp4-packed"], default="bf16",
                    help="projection weights: bf16, fp8 (W8A8 e4m3), mxfp4 (OCP MXFP4 for the low-batch decode GEMV, "
                         "with a resident bf16 copy for every other kernel) or mxfp4-packed (the same numbers without "
                         "the copy: 4.25 bits per weight resident, expanded into one scratch in front of the bf16 GEMMs)")
    ap.add_argument("--fp8-a16-rows", type=int, default=None,
                    help="fp8 weights: the largest step (rows, 0-64) that runs on bf16 activations (W8A16); above 2 "
                         "the skinny MFMA GEMM's fp8-weight mode takes the steps it has a route for (default: "
                         "CHRONOS_W8A16_ROWS, else 2)")
    ap.add_argument("--max-logprobs", type=int, default=20,
                    help="most top_logprobs a request may ask for (0-20); 0 = logprobs are not offered")
    ap.add_argument("--penalty-window", type=int, default=64,
                    help="history window of repeat / frequency / presence penalties, the most repeat_last_n can "
                         "reach (0-1024); 0 = penalties are not offered")
    ap.add_argument("--embed-pooling", choices=["mean", "last"], default="mean",
                    help="how /api/embed pools the final-norm hidden states: mean over all tokens (takes no prefix-cache "
                         "hit) or the last token's (reuses cached prefix blocks)")
    ap.add_argument("--roctx", action="store_true", help="emit roctx ranges for rocprofv3 --marker-trace")
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    if a.roctx:
        from ...utils import trace

        trace.enable()
    logging.basicConfig(level=logging.INFO)
    METRICS.jsonl_path = a.jsonl
    if a.fake:
        backend = FakeBackend(a.fake, delay=60.0)
    else:
        from ..engine.engine import EngineConfig

        cfg = EngineConfig(model=a.model, checkpoint=a.checkpoint, tokenizer=a.tokenizer, device=a.device,
                           max_slots=a.max_slots, max_model_len=a.max_model_len, kv_dtype=a.kv_dtype,
                           weight_dtype=a.weights,
                           **({} if a.fp8_a16_rows is None else {"fp8_a16_rows": a.fp8_a16_rows}),
                           request_timeout_s=a.request_timeout, tp_sequence_parallel=a.sequence_parallel,
                           max_logprobs=a.max_logprobs, penalty_window=a.penalty_window,
                           embed_pooling=a.embed_pooling)
        if a.tp > 1 or a.cp > 1:
            if a.tp > 1 and a.cp > 1:
                raise SystemExit("--tp and --cp are exclusive (CP ranks hold full weights)")
            from ...parallel.tp import TPContext
            from ...parallel.tp_engine import TPEngine, init_tp
            from .service import LockstepService

            if a.device == "cuda":  # before the process group: RCCL and the IPC all-reduce bind the current device
                import torch

                torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
            grp, ctrl = init_tp("nccl" if a.device == "cuda" else "gloo", ipc_allreduce=None if a.tp > 1 else False)
            want = a.tp if a.tp > 1 else a.cp
            if grp.world != want:
                raise SystemExit(f"world size {grp.world} != {'--tp' if a.tp > 1 else '--cp'} {want}")
            tpe = TPEngine(cfg, grp, ctrl) if a.tp > 1 else TPEngine(cfg, TPContext.single(), ctrl, cp=grp)
            if grp.rank != 0:
                freeze_startup_objects()
                tpe.follower_loop()  # until the leader shuts down
                return 0
            def fatal(e):  # the group is out of lockstep: exit non-zero so the supervisor restarts every rank
                log.error("lockstep group failed (%s); exiting so the group restarts", e)
                threading.Timer(2.0, lambda: os._exit(3)).start()  # let /healthz answer 503 meanwhile

            backend = LockstepService(tpe, a.served_name, on_fatal=fatal)
        elif a.dp > 1:
            from ...parallel.router import DPRouter

            backend = DPRouter(cfg, a.dp)
        else:
            from .service import EngineService

            backend = EngineService.from_config(cfg, a.served_name)
    freeze_startup_objects()  # after the engine is built: no full-GC walks over start-up objects
    app = make_app(backend, a.served_name, a.request_timeout or None)
    web.run_app(app, host=a.host, port=a.port, access_log=None)
    return 0
