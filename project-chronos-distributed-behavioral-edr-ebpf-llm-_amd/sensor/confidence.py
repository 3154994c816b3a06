"""How sure was the Brain of its verdict: the probability the model gave to the ``"verdict"`` value it wrote.

The Brain's reply can carry per-token logprobs (``"logprobs": true``, brain/api/protocol.py): for every generated
token, the log-probability among the tokens the verdict grammar allowed at that point.  The tokens that spell the
value of ``"verdict"`` are the one real decision in a verdict (``"SAFE"`` versus ``"MALICIOUS"``: everything around it
is forced by the schema), so the product of their probabilities is the model's confidence in that decision.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence


def _verdict_span(data: bytes) -> Optional[tuple[int, int]]:
    """Byte range [a, b) of the string value of the top-level key "verdict" (between its quotes), or None."""
    depth, i, n = 0, 0, len(data)
    key: Optional[bytes] = None      # the last top-level key seen, while its value has not started
    after_colon = False
    while i < n:
        c = data[i:i + 1]
        if c == b'"':
            j = i + 1
            while j < n and data[j:j + 1] != b'"':
                j += 2 if data[j:j + 1] == b"\\" else 1
            if j >= n:
                return None  # unterminated string
            if depth == 1 and after_colon:
                if key == b"verdict":
                    return i + 1, j
                key, after_colon = None, False
            elif depth == 1:
                key = data[i + 1:j]
            i = j + 1
            continue
        if c in b"{[":
            depth += 1
            if depth > 1:
                key, after_colon = None, False
        elif c in b"}]":
            depth -= 1
        elif c == b":" and depth == 1 and key is not None:
            after_colon = True
        elif c == b"," and depth == 1:
            key, after_colon = None, False
        elif not c.isspace() and depth == 1 and after_colon:
            key, after_colon = None, False  # a number / literal value
        i += 1
    return None


def verdict_confidence(response_text: str, logprobs: Optional[Sequence[dict]]) -> Optional[float]:
    """exp(sum of the logprobs of the tokens that overlap the value of ``"verdict"`` in ``response_text``).

    ``logprobs``: the reply's list of ``{"token", "logprob", "bytes", ...}`` entries, whose ``bytes`` concatenate to
    the response's UTF-8.  None when the reply has no logprobs, the response has no string verdict, or the tokens do
    not cover the verdict (a reply trimmed at a stop string)."""
    if not logprobs:
        return None
    span = _verdict_span(response_text.encode("utf-8"))
    if span is None:
        return None
    a, b = span
    pos, total, covered = 0, 0.0, a
    for e in logprobs:
        nb = len(e.get("bytes") or str(e.get("token", "")).encode("utf-8"))
        lo, hi = pos, pos + nb
        pos = hi
        if hi <= a or nb == 0:
            continue
        if lo >= b:
            break
        lp = e.get("logprob")
        if lp is None:
            return 0.0  # a -inf logprob (JSON null)
        total += float(lp)
        covered = max(covered, min(hi, b))
    if a < b and covered < b:
        return None
    return math.exp(total)
