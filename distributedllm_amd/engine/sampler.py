"""Token sampler — exact behavioral parity with the reference Sampler
(/root/reference/distllm/cli_api/common.py:64-86):

* every previously sampled id gets its logit DIVIDED by the repetition
  penalty (including the negative-logit quirk: dividing a negative logit
  makes it LESS negative, i.e. the "penalty" boosts negative logits —
  reproduced deliberately for behavioral compatibility),
* all logits divide by (temperature + 1e-5),
* softmax then categorical draw (numpy RNG).

A greedy mode mirrors the engine's device argmax semantics. Optional
``top_k``/``top_p`` (nucleus) filtering extends the reference surface
(off by default — defaults are exact reference behavior).

`logprobs_reference` is the float64 definition of the per-token
log-probabilities the serving surfaces report.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np


def softmax(x: np.ndarray) -> np.ndarray:
    x = x - x.max()
    e = np.exp(x)
    return e / e.sum()


class Sampler:
    EPS = 1e-5

    def __init__(self, temperature: float = 0.7, repeat_penalty: float = 1.1,
                 seed: Optional[int] = None, greedy: bool = False,
                 top_k: int = 0, top_p: float = 1.0):
        self.T = temperature
        self.penalty = repeat_penalty
        self.previous_ids: List[int] = []
        self.greedy = greedy
        self.top_k = top_k      # 0 = off
        self.top_p = top_p      # 1.0 = off
        self.rng = np.random.default_rng(seed)

    def __call__(self, logits) -> int:
        logits = np.asarray(logits, dtype=np.float64).reshape(-1)
        if self.greedy:
            tid = int(np.argmax(logits))
            self.previous_ids.append(tid)
            return tid
        size = logits.shape[0]
        mask = np.isin(np.arange(size), self.previous_ids)
        penalties = (mask * self.penalty + ~mask) * (self.T + self.EPS)
        probs = softmax(logits / penalties)
        if self.top_k and self.top_k < size:
            kth = np.partition(probs, -self.top_k)[-self.top_k]
            probs = np.where(probs >= kth, probs, 0.0)
            # renormalize before the nucleus cut: sequential-filter
            # semantics (llama.cpp/HF renormalize between filters) —
            # without this, top_p over the <1 surviving mass keeps a
            # different set, and top_p > surviving mass is a no-op
            probs = probs / probs.sum()
        if self.top_p < 1.0:
            order = np.argsort(-probs)
            csum = np.cumsum(probs[order])
            # keep the smallest prefix whose mass reaches top_p
            cut = int(np.searchsorted(csum, self.top_p) + 1)
            keep = np.zeros(size, dtype=bool)
            keep[order[:cut]] = True
            probs = np.where(keep, probs, 0.0)
        if self.top_k or self.top_p < 1.0:
            probs = probs / probs.sum()
        tid = int(self.rng.choice(size, p=probs))
        self.previous_ids.append(tid)
        return tid

    def draw_params(self):
        """Next uniform of this request's RNG stream plus the filter
        settings: (u, temperature, repeat_penalty, top_k, top_p). Drives
        `sample_reference` / the engines' device `sample` from the same
        object `__call__` serves; the caller appends the chosen id to
        `previous_ids`."""
        return (float(self.rng.random()), float(self.T),
                float(self.penalty), int(self.top_k), float(self.top_p))


def reference_probs(logits, prev_ids, temperature, repeat_penalty, top_k,
                    top_p, dtype=np.float64):
    """The distribution `sample_reference` draws from (steps 1-4 of its
    docstring): filtered, renormalised probabilities over the vocabulary,
    zero outside the kept set."""
    logits = np.asarray(logits, dtype=dtype).reshape(-1)
    size = logits.shape[0]
    mask = np.zeros(size, dtype=bool)
    if len(prev_ids):
        mask[np.asarray(prev_ids, dtype=np.int64)] = True
    penalties = ((mask * dtype(repeat_penalty) + ~mask) *
                 (dtype(temperature) + dtype(Sampler.EPS)))
    probs = softmax(logits / penalties)
    if top_k and top_k < size:
        kth = np.partition(probs, -top_k)[-top_k]
        probs = np.where(probs >= kth, probs, 0.0)
        probs = probs / probs.sum()
    if top_p < 1.0:
        order = np.argsort(-probs, kind="stable")
        csum = np.cumsum(probs[order])
        cut = min(int(np.searchsorted(csum, top_p)), size - 1)
        tau = probs[order[cut]]
        probs = np.where((probs >= tau) & (probs > 0), probs, 0.0)
    if top_k or top_p < 1.0:
        probs = probs / probs.sum()
    return probs


def sample_reference(logits, u, prev_ids, temperature, repeat_penalty,
                     top_k, top_p, dtype=np.float64):
    """Pure form of `Sampler.__call__` driven by one uniform `u` in
    [0, 1): returns (token, kept_mask). These are the semantics the
    device sampling kernel is checked against.

    1. z_i = logit_i / (pen_i * (T + 1e-5)), pen_i = repeat_penalty for
       ids in `prev_ids`, else 1 (negative logits are boosted, as in
       `Sampler`).
    2. p = softmax(z).
    3. top_k (0 or >= V: off): keep p_i >= the k-th largest value, ties
       at the threshold all kept; renormalise.
    4. top_p (>= 1: off): tau = the largest value whose mass {p >= tau}
       reaches top_p; keep p_i >= tau, ties all kept; renormalise. The
       threshold form of "smallest sorted prefix" - equal to `Sampler`
       whenever no tie sits on the boundary.
    5. first index whose cumulative kept probability exceeds u - the
       draw `Generator.choice(size, p=probs)` makes from
       `Generator.random()`. A token outside the kept set is never
       returned.
    """
    probs = reference_probs(logits, prev_ids, temperature, repeat_penalty,
                            top_k, top_p, dtype)
    size = probs.shape[0]
    cdf = np.cumsum(probs)
    cdf = cdf / cdf[-1]
    tid = int(np.searchsorted(cdf, u, side="right"))
    kept = probs > 0
    if tid >= size or not kept[tid]:
        # u within rounding of 1: the last kept token
        tid = int(np.flatnonzero(kept)[-1])
    return tid, kept


LOGPROBS_MAX_TOP = 8   # kernels.h; the serving surfaces accept 0..8


def logprobs_reference(logits_row, token_id, top_n=0):
    """Log-probability of `token_id` under softmax of the RAW logits row
    (full vocabulary, float64): (lp, top_ids[top_n], top_lp[top_n]).

    Temperature, repetition penalty, top-k and top-p do not enter - the
    OpenAI convention: log-probabilities describe the model, not the
    sampler. `top_ids` are the `top_n` largest logits in descending
    order, a tie resolving to the smaller index (the device argmax rule);
    `top_lp` their log-probabilities. A -inf logit has log-probability
    -inf. These are the semantics the device logprobs kernel is checked
    against."""
    x = np.asarray(logits_row, dtype=np.float64).reshape(-1)
    size = x.shape[0]
    top_n = int(top_n)
    if top_n < 0 or top_n > size:
        raise ValueError(f"top_n={top_n} outside 0..V={size}")
    token_id = int(token_id)
    if not 0 <= token_id < size:
        raise ValueError(f"token id {token_id} outside the vocabulary")
    m = x.max()
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = m + np.log(np.exp(x - m).sum())
        # stable sort of the negated row: descending, equal values in
        # index order
        top_ids = np.argsort(-x, kind="stable")[:top_n].astype(np.int64)
        top_lp = x[top_ids] - lse
        lp = float(x[token_id] - lse)
    return lp, top_ids, top_lp


def score_reference(logits_rows, targets):
    """Prompt scoring in float64: row t of `logits_rows` [T, V] scored
    against `targets[t]` - (lp [T], top_id [T], top_lp [T]).

    `lp[t]` is the log-softmax value of the target under the raw logits,
    `top_id[t]` the row's arg-max (a tie resolves to the smaller index) and
    `top_lp[t]` its log-probability: `logprobs_reference(row, target, 1)`
    row by row. A target outside [0, V) means "no target for this row":
    `lp[t]` is NaN, the top entry is still reported. These are the
    semantics the engines' `score()` is checked against."""
    x = np.asarray(logits_rows, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("score_reference: logits_rows must be [T, V]")
    tg = np.asarray(targets, dtype=np.int64).reshape(-1)
    n, size = x.shape
    if tg.shape[0] != n:
        raise ValueError("score_reference: one target per row")
    lp = np.full(n, np.nan)
    top_id = np.empty(n, dtype=np.int64)
    top_lp = np.empty(n)
    for t in range(n):
        ok = 0 <= tg[t] < size
        v, ids, lps = logprobs_reference(x[t], tg[t] if ok else 0, 1)
        if ok:
            lp[t] = v
        top_id[t], top_lp[t] = ids[0], lps[0]
    return lp, top_id, top_lp
