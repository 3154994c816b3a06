"""Ollama REST protocol pieces.

The sensor's request (reference chronos_sensor.py:117-119):
    POST /api/generate {"model": "llama3", "prompt": ..., "stream": false, "format": "json"}
and it reads ``json.loads(resp.json()["response"])`` (:120).  Ollama's other generate fields (system, raw, options,
stream=true NDJSON, timing fields in ns) and /api/chat are served too so any Ollama client can talk to the Brain:

* ``options.stop`` (string or list): generation ends at the first stop string, which is not part of the response;
* ``options.num_ctx``: the request's context window (prompt + generation), clamped to the engine's max_model_len — a
  prompt that does not fit is a 400, ``num_predict`` is clamped to what is left;
* ``context`` (request) continues from a previous reply's ``context`` (returned: prompt + generated token ids);
* ``keep_alive`` is accepted; the weights stay resident regardless (warm at start-up, quirk X8);
* ``options.repeat_penalty`` / ``frequency_penalty`` / ``presence_penalty`` / ``repeat_last_n`` are llama.cpp's
  penalties, applied on the device inside the decode step (csrc/kernels/penalties.hip).  At every sampler step the
  history is the last ``repeat_last_n`` tokens of the prompt followed by everything generated so far (grammar-forced
  tokens included); each distinct token ``v`` of it with count ``c`` gets ``x = logit[v]; x = x * repeat_penalty if
  x <= 0 else x / repeat_penalty; x -= c * frequency_penalty + presence_penalty``.  Legality (``format``, budget
  forcing) is not affected: a forced token stays forced.  The defaults are neutral (1 / 0 / 0) — Ollama's own default
  ``repeat_penalty`` of 1.1 is deliberately NOT applied, so a request that names no penalty decodes as it always did.
  ``repeat_last_n`` defaults to 64; 0 switches the penalties off for the request; -1 means as far back as the engine
  keeps; any value above the engine's window (``--penalty-window``, EngineConfig.penalty_window, at most 1024) is
  clamped to that window.  A backend that cannot apply them (server started with ``--penalty-window 0``, the fake
  backend) answers normally, unpenalised, and names each penalty that is not neutral in ``ignored_options``;
* ``options.min_p`` (0..1, default 0 = off) and ``options.typical_p`` (above 0 up to 1, default 1 = off) are
  llama.cpp's truncation samplers, applied on the device inside the decode step (csrc/kernels/truncate.hip) to the
  raw logits of the *legal set* (below), before temperature, and only when the request samples (temperature > 0:
  greedy ignores them as it ignores top_k / top_p).  typical_p: with ``p = softmax(logit)`` over the legal tokens and
  entropy ``H``, tokens are taken by ascending ``|-log p(v) - H|`` until their accumulated probability exceeds
  ``typical_p``; every token at most as far from ``H`` as the last one taken survives (ties kept: equal logits share
  their fate, at least one token survives).  min_p, after it: a token survives iff ``p(v) >= min_p * p(best
  survivor)``, computed as ``logit[v] >= max logit of the survivors + ln(min_p)``; ``min_p: 1`` keeps only the
  maxima.  The others are masked (-inf) before the sampler.  A grammar-forced token (one legal token) stays forced.
  Ordering deviation from llama.cpp, whose chain is top_k -> typical_p -> top_p -> min_p: here top_k / top_p stay in
  the sampler kernel, so the chain is typical_p -> min_p -> top_k -> top_p, each acting on the survivors of the one
  before.  A backend that cannot apply them (the fake backend) names the non-neutral ones in ``ignored_options``;
* ``options.mirostat: 2`` (the integer) is Mirostat 2.0, llama.cpp's ``llama_sampler_mirostat_v2``, with
  ``options.mirostat_tau`` (target surprise in bits, default 5.0) and ``options.mirostat_eta`` (learning rate,
  default 0.1), both finite numbers >= 0 (a 400 that names the option otherwise).  It runs on the device inside the
  decode step (csrc/kernels/mirostat.hip), over the *legal set* (below) and after the request's penalties, when the
  request samples (temperature T > 0; at temperature 0 the request is greedy, mirostat is neutral and nothing is
  reported, the same rule as min_p / typical_p).  Per sampled token, with ``m`` the largest legal logit and
  ``Z = sum exp((logit[u] - m) / T)``: the surprise of ``v`` is ``S(v) = ((m - logit[v]) / T + ln Z) / ln 2`` bits;
  a token survives iff ``S(v) <= mu`` (if none does, the maxima survive; equal logits share their fate), the others
  are masked (-inf), the sampler draws from the survivors at temperature T, and with ``t`` the drawn token and ``Z'``
  the survivors' share of ``Z``: ``mu <- mu - eta * (S_obs - tau)``, ``S_obs = ((m - logit[t]) / T + ln Z') / ln 2``
  (the surprise under the renormalised distribution, as in llama.cpp).  ``mu`` starts at ``2 * tau`` and is not
  clamped (llama.cpp has no clamp).  Decisions taken here:

  - *forced tokens leave mu unchanged* (a deviation from llama.cpp, which books surprise 0 for a forced token and
    so raises ``mu`` by ``eta * tau``): a step with fewer than two legal tokens, or with every legal logit -inf,
    writes nothing.  Under a schema about half of the tokens are forced and ``mu`` would climb until nothing is
    truncated.  It also keeps jump-forward consistent: a forced run appended by the host never passes the sampler
    and does not move ``mu``, so jump-forward stays on for mirostat requests;
  - *mirostat replaces the truncation chain*: as in llama.cpp the chain is penalties -> temperature -> mirostat,
    so ``top_k``, ``top_p``, ``min_p`` and ``typical_p`` of such a request are neutral and none of them is
    reported as ignored: that is the semantics of the option;
  - *logprobs stay untruncated*: they are taken before the mirostat kernel, like before every other truncation;
  - a backend that cannot apply it (the fake backend) names ``mirostat`` and whichever of ``mirostat_tau`` /
    ``mirostat_eta`` were sent in ``ignored_options``;
* ``options.mirostat`` with any other non-zero value (version 1 needs a sorted top-100 and is not implemented;
  ``mirostat_tau`` / ``mirostat_eta`` with it) and ``options.tfs_z`` (other than 1; removed from llama.cpp) are
  not implemented by any backend and are named in ``ignored_options``.

Per-token logprobs (``"logprobs": true`` and optionally ``"top_logprobs": n``, 0 <= n <= 20, both top-level, for
generate and chat).  The reply gains ``"logprobs": [{"token", "logprob", "bytes", "top_logprobs": [{"token",
"logprob", "bytes"}, ...]}, ...]``, one entry per generated token (for chat beside ``message``).  Semantics, for the
token sampled at output index i (csrc/kernels/logprobs.hip computes them on the device, inside the decode step):

* the *legal set* is exactly the sampler's: tokens the request's grammar (``format``) allows in its current state and
  that still let the output close within ``num_predict`` (budget forcing);
* ``logprob(v) = logit[v] - logsumexp(logit[u] for legal u)``: raw logits, natural log, temperature 1, taken BEFORE
  any min_p / typical_p / top-k / top-p truncation but AFTER the request's penalties (above): the penalty kernel
  runs first, the logprob
  kernels and the sampler both see the penalised row, so a request that asks for both gets the logprobs of the
  distribution its token was actually drawn from — whatever the request's temperature, top_k or top_p.  A token the grammar forces (one
  legal token) has logprob exactly 0.0; without a ``format`` this is the ordinary log-softmax (up to budget forcing
  near ``num_predict``);
* ``top_logprobs`` lists the n legal tokens with the largest logits, ordered by logit descending, then token id
  ascending; shorter when fewer than n tokens are legal; alternatives whose logprob is -inf are dropped (JSON cannot
  carry them; a chosen token's -inf would be ``null``);
* ``token`` is the token's bytes decoded as UTF-8 (invalid sequences replaced), ``bytes`` the bytes themselves: the
  ``bytes`` of all entries concatenate to the response's UTF-8;
* with ``stop``, only the entries of tokens that lie wholly inside the returned text are kept;
* deviation from Ollama: with ``stream: true`` the final (``done``) chunk carries the whole list instead of every chunk
  carrying its own tokens', and a streamed reply that is cut at a stop string carries none;
* while a request that wants logprobs is decoding, jump-forward over grammar-forced runs is suppressed for its batch
  (EngineConfig.max_logprobs);
* a backend that cannot produce them (server started with ``--max-logprobs 0``, the fake backend) answers normally and
  names ``"logprobs"`` in ``ignored_options``.

Embeddings (``POST /api/embed`` ``{"model", "input": str | [str], "truncate": true, "options": {"num_ctx"},
"keep_alive"}`` -> ``{"model", "embeddings": [[...], ...], "total_duration", "load_duration", "prompt_eval_count"}``,
and Ollama's legacy ``POST /api/embeddings`` ``{"model", "prompt"}`` -> ``{"embedding": [...]}``, the same vector):

* an input is embedded as a raw prompt: BOS followed by its tokens, no chat template.  An empty string is its BOS-only
  sequence (a deviation: Ollama answers an empty vector for it); ``"input": []`` gives ``"embeddings": []``;
* the vector comes from the *final-RMSNorm hidden state* (the model's last layer output after the final norm, with the
  checkpoint's own norm weight, the state the LM head would read), pooled over the prompt's tokens on the device
  (csrc/kernels/pool.hip) and returned *L2-normalised, fp32* — by both endpoints (a deviation for the legacy one,
  which Ollama does not normalise);
* pooling is the server's choice (``--embed-pooling``, EngineConfig.embed_pooling): ``mean`` (default) is the direction
  of the mean over all tokens — every token's state is needed, so such a request takes no prefix-cache hit;
  ``last`` is the last token's state, which reuses cached prefix blocks like a generate request: the cheap mode for
  event chains behind one long shared instruction prefix;
* ``truncate`` (default true) keeps the first ``num_ctx`` (else max_model_len) tokens of an input that is too long;
  ``truncate: false`` makes that a 400.  ``prompt_eval_count`` is the total over the inputs, after truncation;
  durations are in ns; the order of ``embeddings`` is the order of ``input``;
* 400: a missing ``input`` (``prompt``), one that is neither a string nor a list of strings, a ``truncate`` that is
  not a boolean, a bad ``options.num_ctx``, invalid JSON.  An engine failure is a 500, ``--request-timeout`` a 504;
* a backend that does not embed (tensor / context parallel groups, the data-parallel router, the fake backend)
  answers 501 ``{"error": ...}``; a server started with ``--kv-dtype fp8`` answers 400 with the engine's error
  (embeddings are served with a bf16 KV cache only: e4m3 K / V moves the vectors by 2 - 6 % of their largest component).
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass
from typing import Any, Optional

OLLAMA_VERSION = "0.5.7-chronos"
MAX_TOP_LOGPROBS = 20  # Ollama's cap on top_logprobs (and the kernels': chronos.ops.MAX_TOP_LOGPROBS)
PENALTY_NEUTRAL = (("repeat_penalty", 1.0), ("frequency_penalty", 0.0), ("presence_penalty", 0.0))


def _number(opts: dict, key: str, default: float) -> float:
    """options[key] as a finite float (a 400 that names the option otherwise)."""
    v = opts.get(key, default)
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise BadRequest(f"options.{key} must be a finite number")
    return float(v)


class BadRequest(ValueError):
    pass


@dataclass
class GenerateParams:
    model: str = "llama3"
    prompt: str = ""
    messages: Optional[list] = None
    system: Optional[str] = None
    raw: bool = False
    stream: bool = True
    format: Any = None
    num_predict: int = 0
    temperature: float = 0.0
    seed: int = 0
    top_k: int = 0
    top_p: float = 1.0
    stop: tuple = ()
    num_ctx: int = 0
    context: Optional[list] = None
    keep_alive: Any = None
    # the penalties that are not neutral (none with repeat_last_n 0): reported in ``ignored_options`` by a backend
    # that did not apply them (penalties_ignored)
    ignored: tuple = ()
    repeat_penalty: float = 1.0
    frequency_penalty: float = 0.0
    presence_penalty: float = 0.0
    repeat_last_n: int = 64
    logprobs: int = -1  # -1 = not asked, 0 = the generated tokens' logprobs, n = with the top n alternatives
    min_p: float = 0.0      # 0 = off
    typical_p: float = 1.0  # 1 = off
    mirostat: int = 0  # 2 = Mirostat 2.0; any other value the client sent is 0 here and named in ``unsupported``
    mirostat_tau: float = 5.0
    mirostat_eta: float = 0.1
    mirostat_named: tuple = ()  # with mirostat 2: the mirostat options sent, reported when a backend did not apply it
    # options that no backend implements and that are not at their neutral value: always in ``ignored_options``
    unsupported: tuple = ()

    @classmethod
    def parse(cls, body: dict, chat: bool = False, default_temperature: float = 0.0) -> "GenerateParams":
        if not isinstance(body, dict):
            raise BadRequest("request body must be a JSON object")
        opts = body.get("options") or {}
        if not isinstance(opts, dict):
            raise BadRequest("options must be an object")
        fmt = body.get("format")
        if fmt not in (None, "", "json") and not isinstance(fmt, dict):
            raise BadRequest(f"invalid format {fmt!r}: use \"json\" or a JSON schema object")
        p = cls(
            model=str(body.get("model", "llama3")),
            prompt=str(body.get("prompt", "")),
            system=body.get("system"),
            raw=bool(body.get("raw", False)),
            stream=bool(body.get("stream", True)),  # Ollama's default is streaming
            format=fmt or None,
            num_predict=int(opts.get("num_predict", body.get("num_predict", 0)) or 0),
            temperature=float(opts.get("temperature", default_temperature)),
            seed=int(opts.get("seed", 0) or 0),
        )
        if p.temperature > 0:  # Ollama's sampler defaults apply whenever it samples (top_k 40, top_p 0.9)
            p.top_k = int(opts.get("top_k", 40) or 0)
            p.top_p = float(opts.get("top_p", 0.9))
        stop = opts.get("stop", body.get("stop"))
        if stop is not None:
            stop = [stop] if isinstance(stop, str) else stop
            if not isinstance(stop, list) or not all(isinstance(x, str) for x in stop):
                raise BadRequest("options.stop must be a string or a list of strings")
            p.stop = tuple(x for x in stop if x)
        p.num_ctx = int(opts.get("num_ctx", 0) or 0)
        if p.num_ctx < 0:
            raise BadRequest("options.num_ctx must be positive")
        ctx = body.get("context")
        if ctx is not None:
            if not isinstance(ctx, list) or not all(isinstance(t, int) and t >= 0 for t in ctx):
                raise BadRequest("context must be a list of token ids")
            p.context = ctx
        p.keep_alive = body.get("keep_alive")
        lp, top = body.get("logprobs"), body.get("top_logprobs")
        if lp is not None and not isinstance(lp, bool):
            raise BadRequest("logprobs must be true or false")
        if top is not None:
            if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= MAX_TOP_LOGPROBS:
                raise BadRequest(f"top_logprobs must be an integer from 0 to {MAX_TOP_LOGPROBS}")
            if not lp:
                raise BadRequest("top_logprobs requires logprobs: true")
        if lp:
            p.logprobs = int(top or 0)
        p.repeat_penalty = _number(opts, "repeat_penalty", 1.0)
        if p.repeat_penalty <= 0:
            raise BadRequest("options.repeat_penalty must be greater than 0")
        p.frequency_penalty = _number(opts, "frequency_penalty", 0.0)
        p.presence_penalty = _number(opts, "presence_penalty", 0.0)
        last = opts.get("repeat_last_n", 64)
        if isinstance(last, bool) or not isinstance(last, int) or last < -1:
            raise BadRequest("options.repeat_last_n must be an integer of at least -1")
        p.repeat_last_n = last
        if last != 0:
            p.ignored = tuple(k for k, neutral in PENALTY_NEUTRAL if getattr(p, k) != neutral)
        p.min_p = _number(opts, "min_p", 0.0)
        if not 0.0 <= p.min_p <= 1.0:
            raise BadRequest("options.min_p must be a number from 0 to 1")
        p.typical_p = _number(opts, "typical_p", 1.0)
        if not 0.0 < p.typical_p <= 1.0:
            raise BadRequest("options.typical_p must be a number above 0 and at most 1")
        un = []
        mi = opts.get("mirostat")
        if type(mi) is int and mi == 2:
            p.mirostat = 2
            for k in ("mirostat_tau", "mirostat_eta"):
                v = _number(opts, k, getattr(p, k))
                if v < 0:
                    raise BadRequest(f"options.{k} must be a finite number of at least 0")
                setattr(p, k, v)
            p.mirostat_named = tuple(k for k in ("mirostat", "mirostat_tau", "mirostat_eta") if k in opts)
        elif (mi or 0) != 0:
            un += [k for k in ("mirostat", "mirostat_tau", "mirostat_eta") if k in opts]
        if opts.get("tfs_z", 1) not in (1, None):
            un.append("tfs_z")
        p.unsupported = tuple(un)
        if chat:
            msgs = body.get("messages")
            if not isinstance(msgs, list) or not msgs:
                raise BadRequest("chat requires a non-empty messages list")
            for m in msgs:
                if not isinstance(m, dict) or "role" not in m:
                    raise BadRequest("each message needs a role and content")
            p.messages = msgs
        return p


@dataclass
class EmbedParams:
    model: str = "llama3"
    inputs: tuple = ()
    truncate: bool = True
    num_ctx: int = 0
    legacy: bool = False  # /api/embeddings: one "prompt", one "embedding"

    @classmethod
    def parse(cls, body: dict, legacy: bool = False) -> "EmbedParams":
        if not isinstance(body, dict):
            raise BadRequest("request body must be a JSON object")
        key = "prompt" if legacy else "input"
        if key not in body:
            raise BadRequest(f"missing {key}")
        v = body[key]
        if isinstance(v, str):
            inputs = (v,)
        elif not legacy and isinstance(v, list) and all(isinstance(x, str) for x in v):
            inputs = tuple(v)
        else:
            raise BadRequest("prompt must be a string" if legacy else "input must be a string or a list of strings")
        truncate = body.get("truncate", True)
        if not isinstance(truncate, bool):
            raise BadRequest("truncate must be true or false")
        opts = body.get("options") or {}
        if not isinstance(opts, dict):
            raise BadRequest("options must be an object")
        n = opts.get("num_ctx", 0) or 0
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise BadRequest("options.num_ctx must be a positive integer")
        return cls(str(body.get("model") or "llama3"), inputs, truncate, n, legacy)


def embed_response(model: str, reqs: list, t0: float, legacy: bool = False) -> dict:
    """The /api/embed body (``legacy``: /api/embeddings') from the finished engine requests, in input order."""
    vecs = [[float(x) for x in r.embedding.tolist()] for r in reqs]
    if legacy:
        return {"embedding": vecs[0]}
    return {"model": model, "embeddings": vecs, "total_duration": _ns(time.perf_counter() - t0), "load_duration": 0,
            "prompt_eval_count": sum(len(r.prompt_ids) for r in reqs)}


def chat_prompt_ids(tok, messages: list) -> list:
    """Llama-3 multi-turn chat template."""
    from ..tokenizer import END_HEADER_ID, START_HEADER_ID

    ids = [tok.bos_id]
    for m in messages:
        ids += [START_HEADER_ID] + tok.encode(str(m["role"])) + [END_HEADER_ID]
        ids += tok.encode("\n\n" + str(m.get("content", ""))) + [tok.eot_id]
    ids += [START_HEADER_ID] + tok.encode("assistant") + [END_HEADER_ID] + tok.encode("\n\n")
    return ids


def _ns(s: float) -> int:
    return int(max(0.0, s) * 1e9)


def now_iso() -> str:
    t = time.time()
    return time.strftime("%Y-%m-%dT%H:%M:%S", time.gmtime(t)) + f".{int((t % 1) * 1e6):06d}Z"


def final_fields(req, load_duration: float = 0.0) -> dict:
    first = req.t_first or req.t_done
    return {
        "done": True,
        "done_reason": req.done_reason if req.done_reason != "error" else "stop",
        "total_duration": _ns(req.t_done - req.t_submit),
        "load_duration": _ns(load_duration),
        "prompt_eval_count": len(req.prompt_ids),
        "prompt_eval_duration": _ns(first - (req.t_admit or req.t_submit)),
        "eval_count": len(req.out_ids),
        "eval_duration": _ns(req.t_done - first),
    }


def penalties_ignored(params: GenerateParams, req) -> tuple:
    """The sampling options of ``params`` to report in ``ignored_options``: its non-neutral penalties when the backend
    did not apply them (a finished engine request carries ``penalty``, a tuple, exactly when its engine did), its
    non-neutral ``min_p`` / ``typical_p`` when the backend has no truncation kernel (a finished engine request carries
    ``truncates``; at temperature 0 it is False and nothing is reported: greedy has nothing to truncate), the
    ``mirostat`` options of a ``mirostat: 2`` request when the backend did not apply it (a finished engine request
    carries ``mirostat``, True exactly when its engine did; a request object without the attribute — the fake backend
    — never did; an engine request at temperature 0 is greedy and nothing is reported), and the options no backend
    implements (``params.unsupported``)."""
    pen = () if getattr(req, "penalty", None) else params.ignored
    tr = ()
    if getattr(req, "truncates", None) is None:
        tr = tuple(k for k, neutral in (("min_p", 0.0), ("typical_p", 1.0)) if getattr(params, k) != neutral)
    mi = ()
    if params.mirostat == 2:
        applied = getattr(req, "mirostat", None)
        if applied is None or (not applied and params.temperature > 0):
            mi = params.mirostat_named
    return pen + tr + mi + params.unsupported


def generate_response(model: str, req, ignored: tuple = ()) -> dict:
    d = {"model": model, "created_at": now_iso(), "response": req.text}
    d.update(final_fields(req))
    # Ollama's continuation handle: the tokens of this exchange (template included); send it back as "context"
    d["context"] = [int(t) for t in list(req.prompt_ids) + list(req.out_ids)]
    if ignored:
        d["ignored_options"] = list(ignored)
    return d


def apply_stop(text: str, stop: tuple) -> tuple[str, bool]:
    """Cut ``text`` at the earliest occurrence of any stop string (Ollama: the stop string is not returned)."""
    cut = min((i for i in (text.find(s) for s in stop) if i >= 0), default=-1)
    return (text[:cut], True) if cut >= 0 else (text, False)


def _visible_tokens(tok, out_ids, visible: str) -> tuple[int, int]:
    """(k, pos): the first k generated tokens lie wholly inside ``visible`` and cover its first ``pos`` bytes."""
    table = tok.token_bytes_list()
    vb = visible.encode("utf-8")
    pos, k = 0, 0
    for t in out_ids:
        b = table[t] if 0 <= t < len(table) else b""
        if not b or not vb.startswith(b, pos):
            break
        pos += len(b)
        k += 1
    return k, pos


def stop_context_ids(tok, prompt_ids, out_ids, visible: str) -> list:
    """The continuation ``context`` of a reply cut at a stop string: the prompt, the generated tokens that lie wholly
    inside the text the client received, then the re-tokenised remainder of that text — never the stop string or
    what followed it (a continuation must not condition on text the client never saw)."""
    k, pos = _visible_tokens(tok, out_ids, visible)
    rest = visible.encode("utf-8")[pos:].decode("utf-8", errors="ignore")
    return [int(t) for t in list(prompt_ids) + list(out_ids[:k])] + ([int(t) for t in tok.encode(rest)] if rest else [])


def chat_response(model: str, req, ignored: tuple = ()) -> dict:
    d = {"model": model, "created_at": now_iso(), "message": {"role": "assistant", "content": req.text}}
    d.update(final_fields(req))
    if ignored:
        d["ignored_options"] = list(ignored)
    return d


def logprobs_field(tok, req, visible: Optional[str] = None) -> Optional[list]:
    """The reply's ``logprobs`` list from a finished request's ``out_logprobs`` (module docstring), or None when the
    backend produced none (the caller then reports "logprobs" in ``ignored_options``).  ``visible``: the text
    returned after a stop-string cut — only the tokens wholly inside it keep their entries."""
    if tok is None or getattr(req, "logprobs", -1) < 0:
        return None
    ids, lps = list(req.out_ids), list(getattr(req, "out_logprobs", None) or [])
    if len(lps) != len(ids):
        return None
    if visible is not None:
        k, _ = _visible_tokens(tok, ids, visible)
        ids, lps = ids[:k], lps[:k]
    table = tok.token_bytes_list()

    def entry(t: int, lp: float) -> dict:
        b = table[t] if 0 <= t < len(table) else b""
        return {"token": b.decode("utf-8", errors="replace"), "logprob": lp if math.isfinite(lp) else None,
                "bytes": list(b)}

    out = []
    for t, (lp, top) in zip(ids, lps):
        e = entry(int(t), float(lp))
        e["top_logprobs"] = [entry(int(a), float(v)) for a, v in top if math.isfinite(v)]
        out.append(e)
    return out


class StopFilter:
    """Streaming form of ``apply_stop``: holds back the last (longest stop - 1) characters so a stop string split
    across chunks is still caught, and emits nothing after it."""

    def __init__(self, stop: tuple):
        self.stop = stop
        self.keep = max(len(x) for x in stop) - 1
        self.buf = ""
        self.hit = False

    def feed(self, text: str) -> str:
        if self.hit:
            return ""
        self.buf += text
        cut, hit = apply_stop(self.buf, self.stop)
        if hit:
            self.hit, self.buf = True, ""
            return cut
        if len(self.buf) > self.keep:
            out, self.buf = self.buf[:len(self.buf) - self.keep], self.buf[len(self.buf) - self.keep:]
            return out
        return ""

    def flush(self) -> str:
        out, self.buf = ("" if self.hit else self.buf), ""
        return out
