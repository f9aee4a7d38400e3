"""Continuous batching over one slice engine.

The reference serves exactly one request at a time (its `generate` loop
holds the whole cluster, /root/reference/distllm/cli_api/common.py:94-111,
and node forwards are serialized). This layer is what the MI355X engine's
batched-decode design (JT column tiles, per-sequence KV slots, explicit
pos/seq on every forward — engine_ext.cpp) was built for: many requests
with different prompts and lengths share one decode step, new requests
are admitted into free KV slots the moment one finishes, and every
decode step advances every active request by one token.

Semantics per request match the TCP client's `generate`
(cluster/llm_client.py): prefill `prompt[:-1]`, then decode the last
prompt token at its true position and sample the continuation — greedy
through the engine's device argmax, or per-request host `Sampler`
(reference parity, including repetition penalty over that request's
sampled ids only). With `device_sampling=True` the sampled requests of
a lane go through ONE `engine.sample` launch instead: the logits stay on
the device and only the ids come back. A request submitted with
`logprobs=n` also records each emitted token's log-probability and the n
most likely alternatives: one `engine.logprobs` launch per lane over the
device ids of argmax / sample, results in the same host sync as the ids.
"""
from __future__ import annotations

from collections import deque
from contextlib import nullcontext as _nullctx
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..engine.sampler import LOGPROBS_MAX_TOP, Sampler, logprobs_reference
from .speculative import lookup_draft


@dataclass
class Request:
    rid: int
    prompt: List[int]
    max_new: int
    sampler: Optional[Sampler] = None  # None => greedy device argmax
    eos_id: Optional[int] = None
    out: List[int] = field(default_factory=list)
    done: bool = False
    slot: int = -1        # KV slot while active
    _next_tok: int = -1   # token to feed at _pos on the next step
    _pos: int = -1
    _pf_pos: int = 0      # prompt tokens already prefilled (chunked)
    # None = off; n >= 0: the chosen token's log-probability plus the n
    # most likely tokens, per generated token (index-aligned with `out`)
    logprobs: Optional[int] = None
    out_logprobs: List[float] = field(default_factory=list)
    out_top: List[List[Tuple[int, float]]] = field(default_factory=list)
    # echo: the same two records for the PROMPT tokens, filled as the
    # prefill passes. Index-aligned with `prompt`; entry 0 is None (the
    # first token has no context to be predicted from)
    echo: bool = False
    prompt_logprobs: List[Optional[float]] = field(default_factory=list)
    prompt_top: List[Optional[List[Tuple[int, float]]]] = field(
        default_factory=list)


class ContinuousBatcher:
    """Slot-based scheduler: submit() any time, step() advances every
    active request one token and admits queued requests into free slots.

    A finished request's KV slot is reused immediately — safe because
    the engine's attention streams exactly rows [0, pos) of a slot, so
    a new sequence starting at pos 0 never sees the old one's rows.
    """

    def __init__(self, engine, max_slots: Optional[int] = None,
                 eos_id: Optional[int] = None, engines=None,
                 prefill_chunk: Optional[int] = None,
                 spec_ngram: int = 0, spec_k: int = 0,
                 device_sampling: bool = False):
        """engines: optional list of k weight-sharing clones ("lanes");
        global slot s lives on lane s%k as that clone's local slot s//k,
        and on CUDA each lane's forward runs on its own HIP stream —
        the decode chain is latency-bound, so concurrent lanes overlap
        (same mechanics as the pipeline's stream lanes).

        prefill_chunk: max prompt tokens prefilled per lane per step
        (None = unbounded, maximizes throughput). A bound interleaves
        long-prompt admission with decode steps, so in-flight requests
        keep producing tokens while a long prompt loads (latency
        fairness — Sarathi-style chunked prefill).

        spec_ngram/spec_k: optional prompt-lookup speculation INSIDE the
        shared decode step (both > 0 to enable). Greedy requests whose
        trailing spec_ngram tokens recur earlier in their sequence get
        up to spec_k draft tokens verified in the same forward — the
        drafts are just more (token, pos, seq) rows in the mixed stream
        the engine already tiles (serving/speculative.py has the
        single-stream form and the KV-staleness argument; per-slot
        positions stay strictly sequential, so the same exactness
        guarantee holds per request). Sampled requests always advance
        one token. Token-exact with spec off — asserted in
        tests/test_serving.py.

        device_sampling: sample on the engine instead of the host. Each
        request's `Sampler` still owns the RNG stream and the settings
        (one uniform per step via `Sampler.draw_params`), but
        `Sampler.__call__` never runs and the [rows, V] logits are never
        copied to the host: a lane's sampled rows share one
        `engine.sample` call on the lane's stream, with the repetition
        state kept per lane-local slot on the device. Raises ValueError
        if an engine has no `sample` (the pipeline facade)."""
        self.engine = engine
        self.lanes = engines if engines else [engine]
        k = len(self.lanes)
        per_lane = min(int(getattr(e, "max_batch", 1))
                       for e in self.lanes)
        slots = per_lane * k
        if max_slots is not None:
            slots = min(slots, max_slots)
        self.n_slots = max(1, slots)
        self.eos_id = eos_id
        self.free: List[int] = list(range(self.n_slots))
        self.active: Dict[int, Request] = {}   # slot -> request
        self.queue: deque[Request] = deque()
        self._next_rid = 0
        self._dev = getattr(engine, "device", "cpu")
        self.prefill_chunk = prefill_chunk
        self.spec_ngram = spec_ngram
        self.spec_k = spec_k
        self.prefilling: Dict[int, Request] = {}  # slot -> request
        self.steps_run = 0      # decode steps executed
        self.tokens_out = 0     # tokens emitted (== steps when spec off)
        self._streams = None
        if k > 1 and self._dev == "cuda":
            self._streams = [torch.cuda.Stream() for _ in self.lanes]
        self.device_sampling = bool(device_sampling)
        self._seen = None       # per-lane repetition state
        # set by the first submit(logprobs=...): until then a step does
        # not even look at the requests' logprobs fields
        self._logprobs_seen = False
        if self.device_sampling:
            if not all(hasattr(e, "sample") and
                       hasattr(e, "new_seen_state") for e in self.lanes):
                raise ValueError(
                    "device_sampling needs an engine with sample()")
            self._seen = [e.new_seen_state() for e in self.lanes]

    def _lane(self, slot: int):
        k = len(self.lanes)
        return self.lanes[slot % k], slot // k

    # ------------------------------------------------------------- intake

    def submit(self, prompt_ids: Sequence[int], max_new: int,
               sampler: Optional[Sampler] = None,
               eos_id: Optional[int] = None,
               logprobs: Optional[int] = None,
               echo: bool = False) -> Request:
        """Raises ValueError (before any slot is taken) on an invalid or
        oversized request — the caller can reject it (HTTP 422) without
        the decode loop ever seeing it.

        logprobs: None = off; n in 0..8 records, per generated token, its
        log-probability under the raw logits (`Request.out_logprobs`) and
        the n most likely tokens with theirs (`Request.out_top`) — the
        semantics of `engine.sampler.logprobs_reference`, independent of
        the sampler settings. Needs an engine with `logprobs()`.

        echo: also record the log-probability of every PROMPT token given
        the tokens before it (`Request.prompt_logprobs`, entry 0 None) and
        the `logprobs` most likely tokens at each prompt position
        (`Request.prompt_top`) - `engine.sampler.score_reference` over the
        prefill's own activations, scored on the device by
        `engine.score()`. Requires `logprobs` and an engine with `score()`;
        with echo, `max_new=0` is a pure scoring request that finishes
        when its prefill does."""
        if logprobs is not None:
            if isinstance(logprobs, bool) or not isinstance(logprobs, int) \
                    or not 0 <= logprobs <= LOGPROBS_MAX_TOP:
                raise ValueError(
                    f"logprobs must be an integer in 0..{LOGPROBS_MAX_TOP}")
            if not all(hasattr(e, "logprobs") for e in self.lanes):
                raise ValueError("logprobs needs an engine with logprobs()")
            self._logprobs_seen = True
        if echo:
            if logprobs is None:
                raise ValueError("echo needs logprobs to be set")
            if not all(hasattr(e, "score") for e in self.lanes):
                raise ValueError("echo needs an engine with score()")
        if len(prompt_ids) < 1:
            raise ValueError("prompt must contain at least one token")
        if max_new < 1 and not (echo and max_new == 0):
            raise ValueError("max_new must be >= 1")
        n_ctx = getattr(self.engine, "n_ctx", None)
        if n_ctx is not None and len(prompt_ids) + max_new > n_ctx:
            raise ValueError(
                f"prompt ({len(prompt_ids)}) + max_new ({max_new}) "
                f"exceeds n_ctx={n_ctx}")
        r = Request(rid=self._next_rid, prompt=list(map(int, prompt_ids)),
                    max_new=max_new, sampler=sampler,
                    eos_id=self.eos_id if eos_id is None else eos_id,
                    logprobs=logprobs, echo=bool(echo))
        if r.echo:
            r.prompt_logprobs.append(None)
            r.prompt_top.append(None)
        self._next_rid += 1
        self.queue.append(r)
        return r

    def _admit(self) -> List[Request]:
        """Returns the requests that finished during admission: pure
        scoring requests (echo, max_new == 0) whose prefill completed."""
        finished: List[Request] = []
        eng = self.engine  # n_ctx/bounds source; lanes share hparams
        n_ctx = getattr(eng, "n_ctx", 1 << 30)
        k = len(self.lanes)
        # take queued requests into free slots; their prompt body
        # prefills below (possibly across several steps when chunked)
        while self.free and self.queue:
            r = self.queue.popleft()
            # submit() already validated against n_ctx; this is a cheap
            # backstop against an engine swap shrinking n_ctx after
            # submission — drop the request rather than corrupt the KV
            if len(r.prompt) + r.max_new > n_ctx:
                r.done = True
                continue
            r.slot = self.free.pop()
            r._pf_pos = 0
            if len(r.prompt) > 1:
                self.prefilling[r.slot] = r
            else:
                self._prefilled(r, finished)
        # prefill as ONE concatenated (token, pos, seq) stream per lane
        # — the engine tiles any mixed-sequence stream internally, so
        # several prompts share each prefill launch; with prefill_chunk
        # set, each lane advances at most that many prompt tokens per
        # step and decode of OTHER requests interleaves
        budget_full = self.prefill_chunk
        scored = []   # per lane with echo rows: _score_lane's result
        per_lane: List[List[Request]] = [[] for _ in range(k)]
        for slot in sorted(self.prefilling):
            per_lane[slot % k].append(self.prefilling[slot])
        for j, reqs in enumerate(per_lane):
            if not reqs:
                continue
            budget = budget_full
            toks, pos, seq = [], [], []
            echo = []   # (request, first stream row, row count)
            for r in reqs:
                end = len(r.prompt) - 1
                take = end - r._pf_pos
                if budget is not None:
                    take = min(take, budget)
                    budget -= take
                if take <= 0:
                    continue
                if r.echo:
                    echo.append((r, len(toks), take))
                toks += r.prompt[r._pf_pos:r._pf_pos + take]
                pos += list(range(r._pf_pos, r._pf_pos + take))
                seq += [r.slot // k] * take
                r._pf_pos += take
            if not toks:
                continue
            lane_eng = self.lanes[j]
            # prefill on the lane's stream: the lane's next decode
            # launch must observe these KV writes, and same-stream
            # ordering gives that without a sync
            ctx = (torch.cuda.stream(self._streams[j])
                   if self._streams is not None else _nullctx())
            with ctx:
                t = torch.tensor(toks, dtype=torch.int32,
                                 device=self._dev)
                p = torch.tensor(pos, dtype=torch.int32,
                                 device=self._dev)
                q = torch.tensor(seq, dtype=torch.int32,
                                 device=self._dev)
                y = lane_eng.forward(lane_eng.embed(t), p, q)
                if echo:
                    scored.append(self._score_lane(lane_eng, y, echo))
        if scored:
            if self._streams is not None:
                for st in self._streams:
                    torch.cuda.current_stream().wait_stream(st)
            for item in scored:
                self._record_echo(*item)
        for slot in list(self.prefilling):
            r = self.prefilling[slot]
            if r._pf_pos >= len(r.prompt) - 1:
                del self.prefilling[slot]
                self._prefilled(r, finished)
        return finished

    def _prefilled(self, r: Request, finished: List[Request]) -> None:
        """The prompt body is in the KV cache: start decoding, or finish
        a pure scoring request (max_new == 0) without activating it."""
        if r.max_new > 0:
            self._activate(r)
            return
        r.done = True
        self.free.append(r.slot)
        r.slot = -1
        finished.append(r)

    def _score_lane(self, eng, y, echo):
        """Score the echo rows of one lane's prefill output `y` on the
        current (the lane's) stream: stream row i of a request's span
        holds prompt position _pf_pos_before + i and is scored against
        the NEXT prompt token. One engine.score call over the gathered
        rows; requests with logprobs >= 2 add logits() + logprobs() over
        their rows for the further alternatives. Returns (echo, packed
        [R, 3] device tensor lp | top_lp | top_id bits, n_top, packed
        [R2, 2 n_top] or None, {echo index: first row in the second})."""
        rows, targets = [], []
        for r, first, take in echo:
            p0 = r._pf_pos - take
            rows += range(first, first + take)
            targets += r.prompt[p0 + 1:p0 + take + 1]
        dev = y.device
        if rows != list(range(y.shape[0])):
            y = y.index_select(0, torch.tensor(rows, dtype=torch.int32,
                                               device=dev))
        tg = torch.tensor(targets, dtype=torch.int32, device=dev)
        lp, top_id, top_lp = eng.score(y, tg)
        packed = torch.stack([lp, top_lp, top_id.view(torch.float32)],
                             dim=1)
        # further alternatives: existing parts over the same rows
        sub, first2, n_top, at = [], {}, 0, 0
        for ei, (r, first, take) in enumerate(echo):
            if r.logprobs >= 2:
                first2[ei] = len(sub)
                sub += range(at, at + take)
                n_top = max(n_top, r.logprobs)
            at += take
        more = None
        if sub:
            if len(sub) != y.shape[0]:
                idx = torch.tensor(sub, dtype=torch.int32, device=dev)
                y, tg = y.index_select(0, idx), tg.index_select(0, idx)
            lg = eng.logits(y, all_logits=True)
            _, ids, lps = eng.logprobs(lg, list(range(len(sub))), tg, n_top)
            more = torch.cat([lps, ids.view(torch.float32)], dim=1)
        return echo, packed, n_top, more, first2

    def _record_echo(self, echo, packed, n_top, more, first2) -> None:
        a = packed.cpu().numpy()
        lp, top_lp = a[:, 0].tolist(), a[:, 1].tolist()
        top_id = a[:, 2].copy().view("int32").tolist()
        if more is not None:
            m = more.cpu().numpy()
            m_lp = m[:, :n_top].tolist()
            m_id = m[:, n_top:].copy().view("int32").tolist()
        at = 0
        for ei, (r, _, take) in enumerate(echo):
            for i in range(at, at + take):
                r.prompt_logprobs.append(lp[i])
                if r.logprobs >= 2:
                    f = first2[ei] + i - at
                    r.prompt_top.append(list(zip(m_id[f][:r.logprobs],
                                                 m_lp[f][:r.logprobs])))
                elif r.logprobs == 1:
                    r.prompt_top.append([(top_id[i], top_lp[i])])
                else:
                    r.prompt_top.append([])
            at += take

    def _activate(self, r: Request) -> None:
        r._next_tok = r.prompt[-1]
        r._pos = len(r.prompt) - 1
        self.active[r.slot] = r
        if self._seen is not None and r.sampler is not None:
            # a reused slot must not inherit the previous request's
            # repetition set; on the lane's stream so it orders with
            # that lane's sample launches
            k = len(self.lanes)
            j = r.slot % k
            ctx = (torch.cuda.stream(self._streams[j])
                   if self._streams is not None else _nullctx())
            with ctx:
                self.lanes[j].reset_seen(self._seen[j], r.slot // k)

    # --------------------------------------------------------------- step

    def step(self) -> List[Request]:
        """Admit what fits, advance every active request one token;
        returns the requests that finished on this step."""
        finished: List[Request] = self._admit()
        if not self.active:
            return finished
        self.steps_run += 1
        k = len(self.lanes)
        # one decode launch per lane, each on its own stream (CUDA)
        per_lane: List[List[int]] = [[] for _ in range(k)]
        for s in sorted(self.active):
            per_lane[s % k].append(s)
        work = []  # (reqs, drafts, greedy_ids, lg, sampled_ids) per lane
        for j, lane_slots in enumerate(per_lane):
            if not lane_slots:
                continue
            reqs = [self.active[s] for s in lane_slots]
            drafts = [self._draft(r) for r in reqs]
            eng = self.lanes[j]
            ctx = (torch.cuda.stream(self._streams[j])
                   if self._streams is not None else _nullctx())
            with ctx:
                if not any(drafts):
                    toks = [r._next_tok for r in reqs]
                    pos = [r._pos for r in reqs]
                    seq = [s // k for s in lane_slots]
                    decode = True   # one row per request, distinct seqs
                else:
                    toks, pos, seq = [], [], []
                    for r, s_, d in zip(reqs, lane_slots, drafts):
                        toks += [r._next_tok] + d
                        pos += list(range(r._pos, r._pos + 1 + len(d)))
                        seq += [s_ // k] * (1 + len(d))
                    decode = False  # same-seq multi-pos rows (mixed
                    #                 admission stream semantics)
                t = torch.tensor(toks, dtype=torch.int32,
                                 device=self._dev)
                p = torch.tensor(pos, dtype=torch.int32,
                                 device=self._dev)
                q = torch.tensor(seq, dtype=torch.int32,
                                 device=self._dev)
                y = eng.forward(eng.embed(t), p, q, decode=decode)
                lg = eng.logits(y, all_logits=True)
                greedy_ids = None
                if any(self._is_greedy(r) for r in reqs):
                    greedy_ids = eng.argmax(lg)
                sampled_ids = None
                if self.device_sampling:
                    sampled_ids = self._sample_lane(eng, j, lg, reqs,
                                                    lane_slots, drafts)
                lp = None
                if self._logprobs_seen and any(r.logprobs is not None
                                               for r in reqs):
                    lp = self._logprobs_lane(eng, lg, reqs, drafts,
                                             greedy_ids, sampled_ids)
            work.append((reqs, drafts, greedy_ids, lg, sampled_ids, lp))
        if self._streams is not None:
            for st in self._streams:
                torch.cuda.current_stream().wait_stream(st)

        for reqs, drafts, greedy_ids, lg, sampled_ids, lp in work:
            if greedy_ids is not None and greedy_ids.device.type != "cpu":
                greedy_ids = greedy_ids.cpu()
            lg_host = None
            if self.device_sampling:
                if sampled_ids is not None:
                    sampled_ids = sampled_ids.cpu().tolist()
            elif any(r.sampler is not None for r in reqs):
                lg_host = lg.float().cpu().numpy()
            if lp is not None:
                # the launch was queued behind the ids on the lane's
                # stream: this copy waits for nothing the id copy above
                # did not already wait for
                packed, n, first = lp
                a = packed.cpu().numpy()
                lp = (a[:, 0].tolist(), a[:, 1:1 + n].tolist(),
                      a[:, 1 + n:].copy().view("int32").tolist(), first)
            self._advance(reqs, drafts, greedy_ids, lg_host, finished,
                          sampled_ids, lp)
        return finished

    def _is_greedy(self, r: Request) -> bool:
        """Served by the engine's argmax: no sampler, or (device
        sampling) a sampler in greedy mode."""
        return r.sampler is None or (self.device_sampling and
                                     r.sampler.greedy)

    def _sample_lane(self, eng, j, lg, reqs, lane_slots, drafts):
        """One engine.sample call for the lane's sampled requests (in
        request order, which _advance consumes); None if there are none.
        Draws each request's next uniform."""
        k = len(self.lanes)
        rows, slots, params = [], [], []
        row = 0
        for r, s_, d in zip(reqs, lane_slots, drafts):
            if not self._is_greedy(r):
                rows.append(row)
                slots.append(s_ // k)
                params.append(r.sampler.draw_params())
            row += 1 + len(d)
        if not rows:
            return None
        u, temp, pen, top_k, top_p = zip(*params)
        return eng.sample(lg, rows, slots, u, temp, pen, top_k, top_p,
                          self._seen[j])

    def _logprobs_lane(self, eng, lg, reqs, drafts, greedy_ids,
                       sampled_ids):
        """One engine.logprobs call for the lane's requests that asked
        and whose token was chosen on the engine (argmax or device
        sample); the chosen ids are gathered on the device. Returns
        (packed [R, 1 + 2n] device tensor: lp ‖ top_lp ‖ top_ids bits, n,
        {request index: its first packed row}), or None when every asker
        is host-sampled (those are served from the host logits)."""
        n_greedy = 0 if greedy_ids is None else int(greedy_ids.shape[0])
        rows, src, first = [], [], {}
        row = 0
        n_sampled = 0
        top_n = 0
        for qi, (r, d) in enumerate(zip(reqs, drafts)):
            greedy = self._is_greedy(r)
            if r.logprobs is not None and (greedy or self.device_sampling):
                first[qi] = len(rows)
                top_n = max(top_n, r.logprobs)
                if greedy:
                    # all 1 + len(draft) rows: row + i holds the token
                    # _advance emits for accepted position i
                    span = range(row, row + 1 + len(d))
                    rows += span
                    src += span
                else:
                    rows.append(row)
                    src.append(n_greedy + n_sampled)
            if not greedy and self.device_sampling:
                n_sampled += 1
            row += 1 + len(d)
        if not rows:
            return None
        parts = [t for t in (greedy_ids, sampled_ids) if t is not None]
        ids = parts[0] if len(parts) == 1 else torch.cat(parts)
        if src != list(range(int(ids.shape[0]))):
            ids = ids.index_select(0, torch.tensor(
                src, dtype=torch.int32, device=ids.device))
        lp, top_ids, top_lp = eng.logprobs(lg, rows, ids, top_n)
        if top_n:
            lp = torch.cat([lp.unsqueeze(1), top_lp,
                            top_ids.view(torch.float32)], dim=1)
        else:
            lp = lp.unsqueeze(1)
        return lp, top_n, first

    def _draft(self, r: Request) -> List[int]:
        """Prompt-lookup draft for a greedy request (possibly empty)."""
        if (self.spec_k <= 0 or self.spec_ngram <= 0 or
                r.sampler is not None):
            return []
        n_ctx = getattr(self.engine, "n_ctx", 1 << 30)
        k = min(self.spec_k, r.max_new - len(r.out) - 1,
                n_ctx - r._pos - 2)
        if k <= 0:
            return []
        return lookup_draft(r.prompt + r.out, self.spec_ngram, k)

    def _advance(self, reqs, drafts, greedy_ids, lg_host,
                 finished, sampled_ids=None, lp=None) -> None:
        row = 0
        n_sampled = 0
        for qi, (r, draft) in enumerate(zip(reqs, drafts)):
            nrows = 1 + len(draft)
            rec = None   # per emitted token: (lp, top ids, top lps)
            if lp is not None and r.logprobs is not None and \
                    qi in lp[3]:
                f = lp[3][qi]
                rec = [(lp[0][f + i], lp[2][f + i], lp[1][f + i])
                       for i in range(nrows)]
            if self.device_sampling and r.sampler is not None:
                if r.sampler.greedy:
                    tid = int(greedy_ids[row])
                else:
                    tid = int(sampled_ids[n_sampled])
                    n_sampled += 1
                r.sampler.previous_ids.append(tid)
                emit = [tid]
            elif r.sampler is not None:
                emit = [r.sampler(lg_host[row])]
                if r.logprobs is not None:
                    # the row is on the host already: no device launch
                    v, top_ids, top_lp = logprobs_reference(
                        lg_host[row], emit[0], r.logprobs)
                    rec = [(v, top_ids.tolist(), top_lp.tolist())]
            else:
                nxt = [int(greedy_ids[row + i]) for i in range(nrows)]
                acc = 0
                while acc < len(draft) and draft[acc] == nxt[acc]:
                    acc += 1
                emit = nxt[:acc + 1]   # verified greedy continuations
            row += nrows
            for i, tid in enumerate(emit):
                self.tokens_out += 1
                r.out.append(tid)
                if rec is not None:
                    v, top_ids, top_lp = rec[i]
                    r.out_logprobs.append(v)
                    r.out_top.append(list(zip(top_ids[:r.logprobs],
                                              top_lp[:r.logprobs])))
                r._next_tok = tid
                r._pos += 1
                if len(r.out) >= r.max_new or (r.eos_id is not None and
                                               tid == r.eos_id):
                    r.done = True
                    del self.active[r.slot]
                    self.free.append(r.slot)
                    r.slot = -1
                    finished.append(r)
                    break

    def cancel(self, req: Request) -> bool:
        """Abort a request: drop it from the queue, or free its slot if
        active (the slot's KV rows are dead — safe to reuse, attention
        is pos-bounded). Returns False if it already finished."""
        if req.done:
            return False
        if req.slot >= 0 and (req.slot in self.active or
                              req.slot in self.prefilling):
            self.active.pop(req.slot, None)
            self.prefilling.pop(req.slot, None)
            self.free.append(req.slot)
            req.slot = -1
        else:
            try:
                self.queue.remove(req)
            except ValueError:
                return False
        req.done = True
        return True

    # --------------------------------------------------------- convenience

    @property
    def pending(self) -> int:
        return len(self.queue) + len(self.active) + len(self.prefilling)

    def run_all(self, max_steps: int = 1 << 20) -> List[Request]:
        """Drive step() until every submitted request finishes."""
        out: List[Request] = []
        for _ in range(max_steps):
            if not self.pending:
                break
            out.extend(self.step())
        assert not self.pending, "run_all hit max_steps with work pending"
        return out
