"""EngineService: runs one Engine on a dedicated scheduler thread and exposes an asyncio API to the HTTP layer.

Single-owner rule: only the scheduler thread touches the engine and its device state; the HTTP event
loop hands requests (and cancellations) over through a queue and gets results back through
``loop.call_soon_threadsafe``.

Failure detection: a watchdog thread flags the service unhealthy when one engine step runs longer
than ``step_deadline_s`` (a hung kernel or collective); ``/healthz`` then answers 503.  A request whose HTTP caller
gave up (server-side timeout, client disconnect) is cancelled in the engine so its slot and KV blocks are reused.
"""
from __future__ import annotations

import asyncio
import logging
import queue
import threading
import time
from typing import Any, AsyncIterator, Optional

from ...utils import trace
from ...utils.metrics import METRICS
from ..engine.engine import Engine, EngineConfig, Request
from .protocol import GenerateParams, chat_prompt_ids

log = logging.getLogger("chronos.service")


class EngineService:
    def __init__(self, engine: Engine, model_name: str = "llama3", step_deadline_s: float = 120.0):
        self.engine = engine
        self.model_name = model_name
        self.step_deadline_s = step_deadline_s
        self._q: "queue.Queue[tuple]" = queue.Queue()
        self._stop = threading.Event()
        self._step_t0: Optional[float] = None  # start of the step in progress (None between steps)
        self.stalled = False
        self.last_error: Optional[str] = None
        self.failures = 0
        self.fail_backoff_s = 0.1
        self._thread = threading.Thread(target=self._loop, name="chronos-scheduler", daemon=True)
        self._watchdog = threading.Thread(target=self._watch, name="chronos-watchdog", daemon=True)
        self.started = time.time()
        self._thread.start()
        self._watchdog.start()

    @property
    def tok(self):
        return self.engine.tok

    @property
    def weight_dtype(self) -> str:
        return self.engine.cfg.weight_dtype

    @property
    def resident_bytes(self) -> int:
        """Weight bytes resident on the device, the packed-only MXFP4 mode's expansion scratch included."""
        w = self.engine.model.w
        return w.nbytes() + w.scratch_nbytes()

    @classmethod
    def from_config(cls, cfg: EngineConfig, model_name: str = "llama3") -> "EngineService":
        return cls(Engine(cfg), model_name)

    # ---- scheduler thread ------------------------------------------------------------------------------------
    def _loop(self) -> None:
        eng = self.engine
        while not self._stop.is_set():
            try:
                block = not eng.has_work()
                item = self._q.get(timeout=0.05) if block else self._q.get_nowait()
            except queue.Empty:
                item = None
            while item is not None:
                self._handle(item)
                try:
                    item = self._q.get_nowait()
                except queue.Empty:
                    item = None
            if eng.has_work():
                t = self._step_t0 = time.perf_counter()
                try:
                    with trace.range("engine.step"):
                        done = eng.step()
                except Exception as e:  # an engine fault fails loudly in health, never silently
                    self._step_failed(e, "engine step failed")
                    continue
                self._step_t0 = None
                METRICS.observe_step(time.perf_counter() - t, eng)
                for r in done:
                    METRICS.observe_request(r)

    def _step_failed(self, e: BaseException, what: str, backoff: bool = True) -> None:
        """A step raised: mark the service stalled (/healthz 503), answer every in-flight request with an error
        (done_reason 'error', so no HTTP caller waits for a reply that will never come), then back off before the
        next step so a persistent fault does not become a hot loop of tracebacks."""
        self._step_t0 = None
        self.failures += 1
        self.last_error = f"{type(e).__name__}: {e}"
        self.stalled = True
        if self.failures == 1 or self.failures % 100 == 0:
            log.exception("%s (failure #%d)", what, self.failures)
        else:
            log.error("%s (failure #%d): %s", what, self.failures, self.last_error)
        failed = self.engine.fail_all(f"engine step failed: {self.last_error}")
        for r in failed:
            METRICS.observe_request(r)
        if backoff:
            self._stop.wait(min(self.fail_backoff_s * (2 ** min(self.failures - 1, 6)), 10.0))

    def _watch(self) -> None:
        while not self._stop.wait(min(1.0, self.step_deadline_s / 4)):
            t0 = self._step_t0
            if t0 is not None and time.perf_counter() - t0 > self.step_deadline_s and not self.stalled:
                self.stalled = True
                self.last_error = f"engine step exceeded {self.step_deadline_s:.0f}s deadline"
                log.error("%s; stats=%s", self.last_error, dict(self.engine.stats))

    def _handle(self, item) -> None:
        kind = item[0]
        if kind == "submit":
            _, params, ids, on_done, on_tokens, handle = item
            if handle.get("cancelled"):  # the caller gave up before admission: never enters the engine
                self.engine.stats["cancelled"] += 1
                return
            handle["req"] = self.engine.submit(
                ids, fmt=params.format, num_predict=params.num_predict, temperature=params.temperature,
                seed=params.seed, top_k=params.top_k, top_p=params.top_p, callback=on_done,
                meta={"on_tokens": on_tokens} if on_tokens else None, max_len=params.num_ctx or None,
                logprobs=params.logprobs, repeat_penalty=params.repeat_penalty,
                frequency_penalty=params.frequency_penalty, presence_penalty=params.presence_penalty,
                repeat_last_n=params.repeat_last_n, min_p=params.min_p, typical_p=params.typical_p,
                mirostat=params.mirostat, mirostat_tau=params.mirostat_tau, mirostat_eta=params.mirostat_eta)
        elif kind == "embed":
            _, text, truncate, num_ctx, on_done, handle = item
            if handle.get("cancelled"):
                self.engine.stats["cancelled"] += 1
                return
            handle["req"] = self.engine.submit_embed(text, max_len=num_ctx or None, truncate=truncate,
                                                     callback=on_done)
        elif kind == "cancel":
            req = item[1].get("req")
            if req is not None and not req.done_reason:
                self.engine.cancel(req)

    def _cancel(self, handle: dict) -> None:
        handle["cancelled"] = True
        self._q.put(("cancel", handle))

    def close(self) -> None:
        self._stop.set()
        self._thread.join(timeout=5)
        self._watchdog.join(timeout=5)

    # ---- asyncio API -------------------------------------------------------------------------------------------
    def _ids(self, params: GenerateParams) -> list:
        tok = self.engine.tok
        if params.messages is not None:
            return chat_prompt_ids(tok, params.messages)
        ids = tok.chat_ids(params.prompt, system=params.system, raw=params.raw)
        if params.context:  # continuation: the previous exchange's tokens, then this turn (without a second BOS)
            ids = list(params.context) + (ids[1:] if ids and ids[0] == tok.bos_id else ids)
        return ids

    async def generate(self, params: GenerateParams) -> Request:
        loop = asyncio.get_running_loop()
        fut: asyncio.Future = loop.create_future()
        handle: dict = {}

        def done(req: Request):
            loop.call_soon_threadsafe(lambda: fut.done() or fut.set_result(req))

        self._q.put(("submit", params, self._ids(params), done, None, handle))
        try:
            return await fut
        except asyncio.CancelledError:  # caller timed out / disconnected: free the engine slot
            self._cancel(handle)
            raise

    async def embed(self, inputs, truncate: bool = True, num_ctx: int | None = None) -> list:
        """One embedding request per input through the scheduler queue (tokenised by the engine at admission); returns
        the finished requests in input order.  A caller that gives up cancels whatever is still in flight."""
        loop = asyncio.get_running_loop()
        futs, handles = [], []
        for text in inputs:
            fut: asyncio.Future = loop.create_future()
            handle: dict = {}

            def done(req: Request, fut=fut):
                loop.call_soon_threadsafe(lambda: fut.done() or fut.set_result(req))

            futs.append(fut)
            handles.append(handle)
            self._q.put(("embed", text, bool(truncate), num_ctx, done, handle))
        try:
            return list(await asyncio.gather(*futs))
        except asyncio.CancelledError:
            for h in handles:
                self._cancel(h)
            raise

    async def generate_stream(self, params: GenerateParams) -> AsyncIterator[tuple[str, Optional[Request]]]:
        """Yields (text_delta, None) pieces, then ("", final_request)."""
        loop = asyncio.get_running_loop()
        aq: asyncio.Queue = asyncio.Queue()
        tok = self.engine.tok
        handle: dict = {}

        def on_tokens(new_ids: list):
            loop.call_soon_threadsafe(aq.put_nowait, ("tok", new_ids))

        def done(req: Request):
            loop.call_soon_threadsafe(aq.put_nowait, ("done", req))

        self._q.put(("submit", params, self._ids(params), done, on_tokens, handle))
        pending = b""
        finished = False
        try:
            while True:
                kind, val = await aq.get()
                if kind == "tok":
                    ids = [i for i in val if i not in tok.stop_ids]
                    pending += b"".join(tok.token_bytes_list()[i] for i in ids)
                    # emit only complete UTF-8 sequences
                    try:
                        text = pending.decode("utf-8")
                        pending = b""
                    except UnicodeDecodeError as e:
                        text = pending[:e.start].decode("utf-8")
                        pending = pending[e.start:]
                    if text:
                        yield text, None
                else:
                    finished = True
                    if pending:
                        yield pending.decode("utf-8", errors="replace"), None
                    yield "", val
                    return
        finally:
            if not finished:  # the consumer stopped early (client went away)
                self._cancel(handle)

    def health(self) -> tuple[bool, dict[str, Any]]:
        busy = self._step_t0
        return not self.stalled, {"status": "stalled" if self.stalled else "ok", "error": self.last_error,
                                  "step_running_s": round(time.perf_counter() - busy, 3) if busy else 0.0}

    def info(self) -> dict[str, Any]:
        eng = self.engine
        return {
            "engines": 1,
            "model": eng.model.cfg.name,
            "params": eng.model.cfg.param_count(),
            "kv_blocks": eng.blocks.num_blocks,
            "kv_free": eng.blocks.free,
            "slots": eng.cfg.max_slots,
            "running": len(eng.running),
            "waiting": len(eng.waiting),
            "stats": dict(eng.stats),
        }


class LockstepService(EngineService):
    """The HTTP-facing service of a TP (or CP) group's leader rank: the same asyncio API and watchdog as
    EngineService, but requests enter the lockstep scheduler (parallel/tp_engine.py TPEngine) and the scheduler
    thread steps it continuously — an idle step is the followers' heartbeat (they block in the step's broadcast).
    Incremental token streaming is not offered here: a stream=true request gets its text in one piece at the end.

    A failed lockstep step is fatal for the group: the followers' engines did not see the leader's failure, so any
    further step would pair the leader's collectives with different ones on the followers (RCCL hang or garbage).
    The leader therefore stops stepping for good, answers every in-flight and later request with an error (the
    reference's ERROR verdict path, chronos_sensor.py:121-122), and calls ``on_fatal`` — the server's default exits
    the process non-zero, which closes the control group so the followers' pending broadcast fails and they exit too;
    the supervisor restarts the whole group in fresh processes (never an exec from a process that touched the GPU)."""

    def __init__(self, tpe, model_name: str = "llama3", step_deadline_s: float = 120.0, idle_s: float = 0.02,
                 on_fatal=None):
        self.tpe = tpe
        self.idle_s = idle_s
        self.broken = False
        self.on_fatal = on_fatal
        super().__init__(tpe.engine, model_name, step_deadline_s)

    embed = None  # embeddings are served at TP = 1 only: the server answers 501 for a backend without ``embed``

    def _error_req(self, ids, reason: str) -> Request:
        r = Request(-1, list(ids), None, 0)
        r.done_reason, r.error = "error", reason
        r.meta["internal_error"] = True
        return r

    def _loop(self) -> None:
        while not self._stop.is_set():
            while True:
                try:
                    self._handle(self._q.get_nowait())
                except queue.Empty:
                    break
            busy = self.engine.has_work()
            t = self._step_t0 = time.perf_counter()
            try:
                done, _ = self.tpe.step()
            except Exception as e:
                self._fatal(e)
                # no further step and no stop broadcast (either would mismatch the followers' collectives), but the
                # thread stays up answering: a request submitted after the failure gets its error reply here
                while not self._stop.is_set():
                    try:
                        self._handle(self._q.get(timeout=0.05))
                    except queue.Empty:
                        pass
                return
            self._step_t0 = None
            if busy:
                METRICS.observe_step(time.perf_counter() - t, self.engine)
            for r in done:
                METRICS.observe_request(r)
            if not busy:
                time.sleep(self.idle_s)
        try:  # release the followers
            self.tpe.step(stop=True)
        except Exception:  # noqa: BLE001 — shutting down
            pass

    def _fatal(self, e: BaseException) -> None:
        self.broken = True
        self._step_failed(e, "lockstep step failed; the TP group must be restarted", backoff=False)
        self.tpe.drop_callbacks()
        while True:  # requests queued behind the failed step never reach the engine
            try:
                item = self._q.get_nowait()
            except queue.Empty:
                break
            if item[0] == "submit":
                item[3](self._error_req(item[2], f"lockstep group failed: {self.last_error}"))
        if self.on_fatal is not None:
            try:
                self.on_fatal(e)
            except Exception:  # noqa: BLE001
                log.exception("on_fatal hook failed")

    def _handle(self, item) -> None:
        kind = item[0]
        if kind == "submit":
            _, params, ids, on_done, _on_tokens, handle = item
            if handle.get("cancelled"):
                return
            if self.broken:
                on_done(self._error_req(ids, f"lockstep group failed: {self.last_error}"))
                return
            handle["tag"] = self.tpe.submit(ids, fmt=params.format, num_predict=params.num_predict,
                                            temperature=params.temperature, seed=params.seed, callback=on_done,
                                            top_k=params.top_k, top_p=params.top_p, max_len=params.num_ctx or None,
                                            logprobs=params.logprobs, repeat_penalty=params.repeat_penalty,
                                            frequency_penalty=params.frequency_penalty,
                                            presence_penalty=params.presence_penalty,
                                            repeat_last_n=params.repeat_last_n, min_p=params.min_p,
                                            typical_p=params.typical_p, mirostat=params.mirostat,
                                            mirostat_tau=params.mirostat_tau, mirostat_eta=params.mirostat_eta)
        elif kind == "cancel":
            tag = item[1].get("tag")
            if tag is not None:
                self.tpe.cancel(tag)

    async def generate(self, params: GenerateParams) -> Request:
        if self.broken:  # the scheduler thread has stopped: answer at once
            return self._error_req(self._ids(params), f"lockstep group failed: {self.last_error}")
        return await super().generate(params)

    def close(self) -> None:
        if self.broken:  # the loop already returned without releasing the followers (they exit with the group)
            self._stop.set()
            self._watchdog.join(timeout=5)
            return
        super().close()

    async def generate_stream(self, params: GenerateParams) -> AsyncIterator[tuple[str, Optional[Request]]]:
        req = await self.generate(params)
        if req.text:
            yield req.text, None
        yield "", req
