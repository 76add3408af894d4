"""Iteration-level scheduling over the engine's paged KV cache (`ContinuousBatcher`) and the prefix cache it can keep (`PrefixCache`).
Needs torch and hashlib only; vita_amd/serving.py puts the vLLM-shaped surface on top and re-exports these names."""
import collections
import hashlib
from dataclasses import dataclass, field
from typing import Any, List, Optional

import torch


def _pages(n_tokens):
    return -(-int(n_tokens) // 64)


@dataclass(slots=True, eq=False)          # eq=False: a request is found in `running` / `waiting` by identity, never by comparing rows
class Request:
    id: Any                                                   # add(): the caller's request id
    emb: torch.Tensor                                         # add(): prompt rows [S, H] fp32; a preemption appends the rows of its output
    max_tokens: int                                           # add(): capped at the engine's max_new
    eos: set = field(default_factory=set)                     # add()
    sampling: Optional[dict] = None                           # add(): keywords of seq_set_sampling without draw0, None for greedy
    rules: Optional[dict] = None                              # add(): keywords of seq_set_logit_rules without the ids, None for none
    prompt_ids: List[int] = field(default_factory=list)       # add(): the prompt set of the penalties
    out: List[int] = field(default_factory=list)              # harvest: every accepted token, across preemptions
    base: int = 0                                             # preemption: len(out) then — the tokens whose rows are part of emb
    seq: Optional[int] = None                                 # _open(): the engine's slot; None again while it waits or once it failed
    hit: int = 0                                              # _open(), with a cache: pages adopted at this admission
    keys: List[bytes] = field(default_factory=list)           # _lookup() / _register_written(): chain keys of the blocks hashed so far
    fresh: bool = False                                       # _start(): the prefill's token is not reported yet; harvest clears it
    done: int = 0                                             # chunked prefill: rows of `suffix` already enqueued (mid-prompt while 0 < done < len)

    @property
    def rows(self):
        return len(self.emb)

    @property
    def suffix(self):                     # the rows that are prefilled: all of them, or what lies behind the pages it adopted
        return self.emb[64 * self.hit:] if self.hit else self.emb

    @property
    def gen(self):                        # the tokens generated since the last (re)prefill
        return self.out[self.base:]


# ---- prefix caching: KV pages of earlier prompts, found again by content -----------------------------------------------------
PREFIX_ROOT_KEY = hashlib.blake2b(b"vita_amd prefix cache v1", digest_size=16).digest()      # key_{-1} of every chain


def chain_keys(digests, cols, parent=PREFIX_ROOT_KEY):
    """digests: the 16-byte content digests of consecutive 64-row blocks (vh_hash_row_blocks) -> their chain keys
    key_b = blake2b(key_{b-1} || digest_b || cols as 8 little-endian bytes, digest_size=16): a key names the WHOLE prefix up to and
    including its block, for rows of that width."""
    keys, tail = [], int(cols).to_bytes(8, "little")
    for d in digests:
        parent = hashlib.blake2b(parent + bytes(d) + tail, digest_size=16).digest()
        keys.append(parent)
    return keys


def device_digests(rows):
    """fp32 [n, H] device rows -> the digests of its complete 64-row blocks as 16-byte strings: ONE vh_hash_row_blocks launch and one
    small device-to-host copy, which waits for the stream — the only synchronisation prefix caching adds."""
    from . import ops
    if len(rows) < 64:
        return []
    words = ops.hash_row_blocks(rows).cpu().numpy()
    return [words[b].tobytes() for b in range(len(words))]


@dataclass(slots=True)
class CacheEntry:
    page: int                             # insert(): the KV page, held once for the cache
    parent: Optional[bytes]               # insert(): the key in front of it, None for block 0
    children: int = 0                     # insert() / evict() of an entry whose parent this is
    tick: int = 0                         # insert() / match(): the cache's tick at its last use


class PrefixCache:
    """Store of the prefix cache (vLLM's enable_prefix_caching over this engine's pages): chain key -> CacheEntry(page, parent key,
    children, last-use tick).  Every entry owns ONE hold of its page (MixtralEngine.seq_hold_prefix), so the page outlives the sequence
    that wrote it; a sequence that adopts it (seq_adopt) adds its own count.  The entries form a forest closed under `parent`: a block
    is cached only together with the whole prefix in front of it.

    Nothing here looks at a clock or iterates a dict of unequal things in hash order: `tick` is a counter the batcher bumps per
    admitted request, eviction orders by (tick, key).  Tensor-parallel ranks fed the same requests reach the same decisions.

    Eviction: only entries whose page has page_refs == 1 (the cache's hold alone), unpinned and without children; least recently
    used first; exactly as many as asked for.

    The device digest is a content hash, not a cryptographic one (include/vita_hip.h vh_hash_row_blocks): a miss is always safe, a
    false hit would not be, which is why the cache is opt-in."""

    def __init__(self, engine, digests=None):
        self.eng, self.digests = engine, digests or device_digests
        self.entries = {}                 # chain key -> CacheEntry
        self.pinned = set()               # pages a request of the current admission pass is about to adopt
        self.tick = self.evictions = 0

    def keys_after(self, keys, rows):
        """keys of the complete blocks of `rows`, which continue the prefix whose keys are `keys`."""
        return chain_keys(self.digests(rows), rows.size(1), keys[-1] if keys else PREFIX_ROOT_KEY)

    def match(self, keys, limit):
        """-> pages of the longest cached chain among the first `limit` keys; the chain is touched."""
        pages = []
        for k in keys[:max(int(limit), 0)]:
            e = self.entries.get(k)
            if e is None:
                break
            e.tick = self.tick
            pages.append(e.page)
        return pages

    def insert(self, key, parent, page):
        """`page` (already held once for the cache) under `key`; parent: the key in front of it, None for block 0."""
        self.entries[key] = CacheEntry(int(page), parent, 0, self.tick)
        if parent is not None:
            self.entries[parent].children += 1

    def _idle(self, e):
        return e.page not in self.pinned and self.eng.page_refs(e.page) == 1

    def evictable(self):
        """entries evict() could remove: idle ones all of whose descendants are idle."""
        blocked = set()
        for k, e in self.entries.items():
            if not self._idle(e):
                while k is not None and k not in blocked:
                    blocked.add(k)
                    k = self.entries[k].parent
        return len(self.entries) - len(blocked)

    def evict(self, n):
        """give up to n pages back to the pool -> how many."""
        done = 0
        while done < n:
            # the least recently used childless idle entry, ties by key; a chain shares one tick and only its leaf is childless: the
            # parent becomes a candidate when the leaf is gone
            leaves = sorted((e.tick, k) for k, e in self.entries.items() if e.children == 0)
            k = next((k for _, k in leaves if self._idle(self.entries[k])), None)
            if k is None:
                break
            gone = self.entries.pop(k)
            if gone.parent is not None:
                self.entries[gone.parent].children -= 1
            self.eng.pages_release([gone.page])
            done += 1
        self.evictions += done
        return done

    def clear(self):
        """drop every entry and its hold (pages a running sequence adopted stay that sequence's until it ends)."""
        pages = sorted(e.page for e in self.entries.values())
        self.entries.clear()
        self.pinned.clear()
        if pages:
            self.eng.pages_release(pages)


# ---- concurrent requests: iteration-level scheduling over the paged KV cache -------------------------------------------
class ContinuousBatcher:
    """The scheduler half of vLLM's engine for this path (what drives the plugin's forward with `kv_caches` +
    `attn_metadata`, vllm_file/mixtral.py:1130-1186), over `MixtralEngine.seq_*`:

      add(request_id, embeds, max_tokens, eos)   queue a request (FIFO)
      step() -> [(request_id, new_token_ids, finished, finish_reason)]   one iteration:
          1. admit waiting requests while a sequence slot is free and the pool holds the prompt's pages plus one page of
             headroom per running sequence; the admitted prompts are then prefilled in groups of up to max_prefill rows, a
             group of two or more in ONE pass over the weights (seq_prefill_batch: vLLM's max_num_batched_tokens), a
             group of one — or a re-prompt longer than max_prefill, in chunks — by seq_prefill;
          2. if the running sequences need more new pages than the pool has, preempt the youngest ones (free their pages,
             re-queue them at the front with prompt + generated tokens as the new prompt: vLLM's recompute preemption);
          3. `window` greedy decode steps for every running sequence (one C call per step), ONE host synchronisation,
             then eos / max_tokens per sequence; finished sequences return their pages.
      abort(request_id)

    A sequence's ids do not depend on what else is scheduled (same kernels, same arithmetic per sequence); tokens decoded
    past an eos inside a window are discarded, as MixtralEngine's single-request lookahead does.

    prefix_cache=True (or a PrefixCache): vLLM's enable_prefix_caching.  On admission the prompt's 64-row blocks are keyed by content
    (one vh_hash_row_blocks launch + one small device-to-host copy per admitted request: the only synchronisation the feature adds);
    the longest cached chain, at most (S - 1) // 64 pages since one row must be prefilled for the first token's logits, is adopted
    (seq_alloc, seq_adopt) and only emb[64 * hit:] is prefilled, as a member of the admission group like any other prompt (it counts
    S - 64 * hit rows against max_prefill).  Right after a request's prefill is enqueued its full prompt pages that are not cached yet
    are held and inserted — everything runs on one stream, so an adopter's kernels are ordered after the writer's; two requests of
    the SAME admission group therefore do not share.  With an embed_tokens hook, a request that finishes, is aborted or is preempted
    also registers its pages that lie entirely below its position, the ones filled by generated tokens included (keys continue the
    chain over cat(open block's prompt rows, embed_tokens(out[:-1]))): a follow-up turn that repeats prompt + response finds them,
    and a preempted request finds its own pages.  Pool accounting is "free + evictable - promised"; cached pages are evicted
    (childless first, least recently used first, exactly as many as needed) before any running sequence is preempted.
    stats: prefix_queries (lookups), prefix_hit_tokens, prefix_evictions, prefill_rows (rows sent to prefill calls, counted with the
    cache off as well).  Side tables by request id, each entry the caller's to pop: errors (the exception behind an "error" event),
    logprobs (per-token {id: logprob} of a request with rules["logprobs"] >= 0) and cached_tokens (the hit of its first admission); a
    request that fails or is aborted loses the last two here (_drop).

    chunked_prefill=True (vLLM's enable_chunked_prefill, on an engine that has seq_step): an iteration that has prompt
    rows is ONE pass over the weights.  Every running sequence takes one row of the budget max_batched_tokens (default and upper
    bound: max_prefill), the rest goes to prompts in admission order — first the request that is mid-prompt, then newly admitted
    ones; a prompt larger than what is left contributes a chunk and its request stays in `prefilling` (it holds its slot and counts
    against max_batch, it is not in `running` and is not harvested) until its last chunk, whose token is its first output: the
    rules are armed in front of that chunk and the prompt's pages are registered with the prefix cache behind it.  One seq_step call
    replaces the prefill call and the first decode step of the window; the other window - 1 steps are seq_decode calls over
    everyone who has a token.  An iteration without prompt rows is today's (seq_decode).  If seq_step raises, the iteration falls
    back to prefill calls and a seq_decode, so that only a culprit fails.  A mid-prompt request yields its slot before any running
    sequence is preempted and re-queues with its full prompt.  stats: mixed_steps (seq_step calls), mixed_rows (their rows);
    prefill_rows counts chunk rows."""

    def __init__(self, engine, embed_tokens=None, max_batch=None, window=1, prefix_cache=False, chunked_prefill=False,
                 max_batched_tokens=None):
        self.eng, self.embed_tokens = engine, embed_tokens
        self.cache = prefix_cache if isinstance(prefix_cache, PrefixCache) else (PrefixCache(engine) if prefix_cache else None)
        self.max_batch = int(max_batch or engine.c.max_seqs)
        if engine.c.max_seqs < 1:
            raise ValueError("the engine was created without sequence slots (max_seqs = 0)")
        self.window = int(window)
        self.budget = int(max_batched_tokens) if max_batched_tokens is not None else int(engine.max_prefill)
        if self.budget > engine.max_prefill:
            raise ValueError(f"max_batched_tokens {self.budget} exceeds the engine's max_prefill {engine.max_prefill}")
        if chunked_prefill and self.budget <= self.max_batch:
            raise ValueError(f"max_batched_tokens {self.budget} leaves no prompt row next to {self.max_batch} running sequences")
        self.chunked = bool(chunked_prefill) and hasattr(engine, "seq_step")
        self.waiting = collections.deque()
        self.running = []                 # admission order
        self.prefilling = []              # chunked prefill: admitted requests whose prompt is not enqueued whole yet, admission order
        self.errors, self.logprobs, self.cached_tokens = {}, {}, {}
        self.stats = {"iterations": 0, "prefills": 0, "prefill_calls": 0, "preemptions": 0, "decode_steps": 0, "failed": 0,
                      "prefix_queries": 0, "prefix_hit_tokens": 0, "prefix_evictions": 0, "prefill_rows": 0}
        if chunked_prefill:               # (the keys exist with the flag on only: with it off the stats are what they were)
            self.stats.update(mixed_steps=0, mixed_rows=0)

    def add(self, request_id, embeds, max_tokens, eos=(), sampling=None, rules=None, prompt_ids=None):
        """sampling: None (greedy) or the keywords of MixtralEngine.seq_set_sampling without draw0 (see sampling_of).
        rules: None or the keywords of MixtralEngine.seq_set_logit_rules without the ids (see rules_of); prompt_ids: the prompt set
        of the penalties.  The rules are re-armed with prompt and output ids after a recompute preemption, and the logprobs of a
        request (self.logprobs[request_id]) run on across it."""
        S = len(embeds)
        if S + 2 > self.eng.max_ctx or S > self.eng.max_prefill:
            raise ValueError(f"prompt of {S} tokens exceeds the engine (max_prefill {self.eng.max_prefill}, pool "
                             f"{self.eng.max_ctx} tokens)")
        self.waiting.append(Request(request_id, embeds, min(int(max_tokens), self.eng.max_new), set(eos), sampling, rules,
                                    list(prompt_ids or ())))
        if rules is not None and rules.get("logprobs", -1) >= 0:
            self.logprobs[request_id] = []

    def _drop(self, request_id):
        """a request ends without finishing: what the scheduler kept for its caller goes"""
        self.logprobs.pop(request_id, None)
        self.cached_tokens.pop(request_id, None)

    def abort(self, request_id):
        self._drop(request_id)
        r = next((r for r in (*self.running, *self.prefilling, *self.waiting) if r.id == request_id), None)
        if r is not None and r in self.prefilling:        # mid-prompt: its slot and pages go back, nothing of it is registered
            self._unslot(r)
        elif r is not None and r.seq is not None:         # running: it holds a slot
            self._retire(r)
        elif r is not None:
            self.waiting.remove(r)
        return r is not None

    def has_work(self):
        return bool(self.waiting or self.running or self.prefilling)

    def _unslot(self, r):
        """a request that is (or may be) mid-prompt gives its slot back"""
        if r in self.prefilling:
            self.prefilling.remove(r)
        if r.seq is not None:
            self.eng.seq_free(r.seq)
        r.seq, r.done, r.hit = None, 0, 0

    def _retire(self, r):
        """a running request ends (finished or aborted): its written pages stay findable, its slot goes back"""
        self._register_written(r)
        self.eng.seq_free(r.seq)
        self.running.remove(r)

    def _prefill(self, r):
        """the prompt of a request — or, after a preemption, prompt + generated tokens, which may exceed what one prefill call
        takes — in chunks of max_prefill (seq_prefill appends at the sequence's position)."""
        emb, mp = r.suffix, int(self.eng.max_prefill)
        for s0 in range(0, len(emb), mp):
            if s0 > 0 and s0 + mp >= len(emb):
                self._arm(r)                 # a chunked re-prompt: only the LAST chunk's token is an output (the table counts it)
            self.eng.seq_prefill(r.seq, emb[s0:s0 + mp])
            self.stats["prefill_calls"] += 1
            self.stats["prefill_rows"] += len(emb[s0:s0 + mp])

    # ---- prefix cache ----------------------------------------------------------------------------------------------------------
    def _lookup(self, r):
        """keys of r's complete prompt blocks (hashed once per prompt; a re-prompt after a preemption only grew) -> the cached pages
        r may adopt, pinned until the admission pass ends."""
        if len(r.keys) < r.rows // 64:
            r.keys += self.cache.keys_after(r.keys, r.emb[64 * len(r.keys):])
        pages = self.cache.match(r.keys, (r.rows - 1) // 64)
        self.cache.pinned.update(pages)
        return pages

    def _register(self, r, n_full):
        """hold r's first n_full pages for the cache, as far as their keys are not cached yet (those form the tail of the chain)."""
        c, keys = self.cache, r.keys
        new = [b for b in range(min(n_full, len(keys))) if keys[b] not in c.entries]
        if not new:
            return
        pages = self.eng.seq_hold_prefix(r.seq, new[-1] + 1)
        if new[0] > 0:
            self.eng.pages_release(pages[:new[0]])             # the hold covers the table's head: the cached part goes back
        for b in new:
            c.insert(keys[b], keys[b - 1] if b else None, pages[b])

    def _register_written(self, r, rows=None):
        """before r's sequence is freed: register its pages that lie entirely below its position, those filled by generated tokens
        included.  rows: r's prompt + embed_tokens(its output), when the caller has built it anyway (preemption)."""
        if self.cache is None or self.embed_tokens is None or r.seq is None:
            return
        gen = r.gen
        # K/V of position S + i is the row of generated token i; the last accepted token was never fed (or its row is discarded)
        valid = min(self.eng.seq_pos(r.seq), r.rows + max(len(gen) - 1, 0))
        if valid // 64 > len(r.keys):
            k0 = 64 * len(r.keys)
            if rows is None:
                tail = self.embed_tokens(torch.tensor(gen[:-1], dtype=torch.long, device=r.emb.device)).to(torch.float32)
                rows = torch.cat([r.emb[k0:], tail], dim=0)
            else:
                rows = rows[k0:]
            r.keys += self.cache.keys_after(r.keys, rows[:64 * (valid // 64) - k0])
        self._register(r, valid // 64)

    # ---- admission ---------------------------------------------------------------------------------------------------------------
    def _arm(self, r):
        """the logit rules of r's slot with its history: the prompt set, and every token generated so far as outputs."""
        if r.rules is not None:
            self.eng.seq_set_logit_rules(r.seq, prompt_ids=r.prompt_ids, output_ids=r.out, **r.rules)

    def _fail(self, r, exc, events):
        """ONE request failed (its prompt does not fit, its prefill was rejected): it ends with an "error" event, nobody else
        is touched; its slot, if it has one, goes back.  Device-level failures (spin time-outs, launch errors) still propagate."""
        self._unslot(r)
        self.errors[r.id] = exc
        self._drop(r.id)
        self.stats["failed"] += 1
        events.append((r.id, [], True, "error"))

    def _promised(self, g):
        """pages of the pool that are promised to the rest of g's prompt"""
        return _pages(g.rows) - (g.hit if g.done == 0 else len(self.eng.seq_pages(g.seq)))

    def _room_for(self, r, group):
        """page accounting for the head of the queue -> the cached pages r adopts (pinned; [] without a cache), None when r has to
        wait for pages, or the error of a prompt that the empty pool cannot hold."""
        # the pool as it will be once the group is prefilled: the pages promised to its prompts are gone, its members run
        # (pages a member adopted from the prefix cache are in its table already)
        free = self.eng.pages_free() - sum(self._promised(g) for g in group)
        n_run = len(self.running) + len(group)
        need = _pages(r.rows + 1) + n_run                           # + one page of headroom per runner
        hit = []
        if self.cache is not None:
            self.cache.tick += 1
            hit = self._lookup(r)
            need -= len(hit)
            if 0 < need - free <= self.cache.evictable():           # free + evictable - promised; the pinned pages are not evictable
                self.stats["prefix_evictions"] += self.cache.evict(need - free)
                free = need
        if need <= free:
            return hit
        if hit:
            self.cache.pinned.difference_update(hit)
        if n_run == 0:
            return RuntimeError(f"request {r.id}: prompt needs {need} KV pages, the pool has {free}")
        return None

    def _open(self, r, hit, events, arm=True):
        """a slot for r with its adopted pages, its sampling and its rules -> True; a failure ends r alone (_fail frees the slot).
        arm=False (chunked prefill): the rules are armed in front of the last chunk, whenever that is."""
        try:
            r.seq = self.eng.seq_alloc()
            if self.cache is not None:
                r.hit = len(hit)
                self.stats["prefix_queries"] += 1
                self.stats["prefix_hit_tokens"] += 64 * len(hit)
                self.cached_tokens.setdefault(r.id, 64 * len(hit))
                if hit:
                    self.eng.seq_adopt(r.seq, hit)
            if r.sampling is not None:
                # draw index of the next token = tokens already generated (r.base after a recompute preemption): the continued
                # ids are the ones an unpreempted run draws
                self.eng.seq_set_sampling(r.seq, draw0=r.base, **r.sampling)
            if arm and len(r.suffix) <= self.eng.max_prefill:        # (a chunked re-prompt arms its rules in front of its last chunk: _prefill)
                self._arm(r)
            return True
        except Exception as e:
            self._fail(r, e, events)
            return False

    def _start(self, r, events, prefilled=False):
        """r holds a slot: prefill it (unless a group call already did) and let it run; a failure ends r alone."""
        if not prefilled:
            try:
                self._prefill(r)
            except Exception as e:
                self._fail(r, e, events)
                return
        r.fresh = True
        self.running.append(r)
        self.stats["prefills"] += 1
        if self.cache is not None:           # the prefill is enqueued: its full prompt pages can be shared from here on
            self._register(r, r.rows // 64)

    def _prefill_group(self, group, events):
        """the admitted requests of one group, in admission order: two or more in one pass over the weights.  A group call that
        raises is retried request by request (a rejected call touched nothing; after a later failure seq_prefill starts again
        at the sequence's unchanged position), so only the culprit ends with an "error" event."""
        done = False
        if len(group) >= 2:
            try:
                self.eng.seq_prefill_batch([r.seq for r in group], [r.suffix for r in group])
                self.stats["prefill_calls"] += 1
                self.stats["prefill_rows"] += sum(len(r.suffix) for r in group)
                done = True
            except Exception:
                pass
        for r in group:
            self._start(r, events, prefilled=done)
        group.clear()

    def _admit(self):
        events = []
        mp = int(self.eng.max_prefill)
        can_batch = hasattr(self.eng, "seq_prefill_batch")
        group = []                # admitted (slot taken, pages promised), prefill deferred to the group's call
        while self.waiting and len(self.running) + len(group) < self.max_batch:
            r = self.waiting[0]
            hit = self._room_for(r, group)
            if hit is None:
                break
            self.waiting.popleft()
            if isinstance(hit, Exception):
                self._fail(r, hit, events)
                continue
            if not self._open(r, hit, events):
                continue
            S = len(r.suffix)
            alone = not can_batch or S > mp      # no batched entry point / a re-prompt that goes in chunks: alone, in order
            if alone or sum(len(g.suffix) for g in group) + S > mp:
                self._prefill_group(group, events)               # ... / r would take the group's rows past max_prefill: close it
            if alone:
                self._start(r, events)
            else:
                group.append(r)
        self._prefill_group(group, events)
        if self.cache is not None:
            self.cache.pinned.clear()
        return events

    def _growth(self, r, steps):
        """pages r's sequence takes from the pool for `steps` more tokens"""
        return _pages(self.eng.seq_pos(r.seq) + steps) - len(self.eng.seq_pages(r.seq))

    def _preempt_for(self, steps):
        """make sure `steps` decode steps of every running sequence find their pages; youngest sequences yield."""
        while True:
            new_pages = sum(self._growth(r, steps) for r in self.running) + sum(self._promised(g) for g in self.prefilling)
            short = new_pages - self.eng.pages_free()
            if short > 0 and self.cache is not None:              # cached pages yield before a running sequence does
                self.stats["prefix_evictions"] += self.cache.evict(short)
                short = new_pages - self.eng.pages_free()
            if short > 0 and self.prefilling and self.running:    # a mid-prompt request (the youngest, nothing produced yet) yields first
                g = self.prefilling[-1]
                self._unslot(g)
                self.waiting.appendleft(g)
                self.stats["preemptions"] += 1
                continue
            if short <= 0 or len(self.running) <= 1:
                return
            r = self.running.pop()
            try:                                                  # the re-prompt's rows -> register what it wrote -> free
                if r.out and self.embed_tokens is None:
                    raise RuntimeError("KV pool exhausted and no embed_tokens hook to recompute a preempted sequence")
                emb = r.emb
                if r.gen:
                    tail = self.embed_tokens(torch.tensor(r.gen, dtype=torch.long, device=emb.device))
                    emb = torch.cat([emb, tail.to(torch.float32)], dim=0)
                self._register_written(r, rows=emb)               # its written pages stay findable: the re-prompt adopts them
            finally:
                self.eng.seq_free(r.seq)                          # (also when there is no hook to recompute it with)
            r.emb, r.base, r.seq = emb, len(r.out), None
            self.waiting.appendleft(r)
            self.stats["preemptions"] += 1

    def _harvest(self, r, starved):
        """the tokens r's sequence produced since the last look: eos / max_tokens, retire it when it ends -> its event or None"""
        cnt = self.eng.check_device_flag(self.eng.seq_counters(r.seq).tolist())
        n_dev = min(cnt[1], self.eng.max_new)                 # tokens of this (re)prefill + its decode steps
        have = len(r.gen)
        new = self.eng.seq_tokens(r.seq)[have:n_dev].tolist()
        new_lp = None
        if r.id in self.logprobs and n_dev > have:
            from .model.vita_mixtral import logprob_dicts
            new_lp = logprob_dicts(tuple(v[have:n_dev] for v in self.eng.logprobs(r.seq)), new, r.rules["logprobs"])
        r.fresh = False
        accepted, reason = [], None
        for tok in new:
            accepted.append(tok)
            if tok in r.eos:
                reason = "stop"
            elif len(r.out) + len(accepted) >= r.max_tokens:
                reason = "length"
            if reason:
                break
        r.out += accepted
        if new_lp is not None:
            self.logprobs[r.id] += new_lp[:len(accepted)]
        if reason is None and (starved or self.eng.seq_pos(r.seq) + 2 >= self.eng.max_ctx):
            reason = "length"                                 # the pool cannot hold another token of this sequence
        if reason:
            self._retire(r)
        if accepted or reason:
            return (r.id, accepted, reason is not None, reason or "")

    # ---- chunked prefill -----------------------------------------------------------------------------------------------------
    def _admit_chunked(self):
        """admission as _admit does it (slot, page accounting over the whole prompt, adoption), without the prefill: the admitted
        requests join `prefilling`.  Nobody is admitted whose first row would not fit this iteration's budget."""
        events = []
        left = self.budget - len(self.running) - sum(len(g.suffix) - g.done for g in self.prefilling)
        while self.waiting and left > 0 and len(self.running) + len(self.prefilling) < self.max_batch:
            r = self.waiting[0]
            hit = self._room_for(r, self.prefilling)
            if hit is None:
                break
            self.waiting.popleft()
            if isinstance(hit, Exception):
                self._fail(r, hit, events)
                continue
            if self._open(r, hit, events, arm=False):
                self.prefilling.append(r)
                left -= len(r.suffix)
        if self.cache is not None:
            self.cache.pinned.clear()
        return events

    def _mixed_pass(self, dec, events):
        """the prompt rows of this iteration and one decode step of the sequences `dec` in ONE pass (seq_step) -> the requests
        whose last chunk it carried (they run from here on)."""
        left = self.budget - len(dec)
        chunks = []                       # (request, rows of its suffix in this pass)
        for g in self.prefilling:
            n = min(len(g.suffix) - g.done, left)
            if n <= 0:
                break
            chunks.append((g, n))
            left -= n
        last = [g for g, n in chunks if g.done + n == len(g.suffix)]
        for g in last:
            self._arm(g)                  # only the LAST chunk's token is an output (the table counts it)
        rows = [g.suffix[g.done:g.done + n] for g, n in chunks]
        try:
            self.eng.seq_step([g.seq for g, _ in chunks], rows, [r.seq for r in dec])
            ok = True
        except Exception:
            ok = False
        if ok:
            self.stats["mixed_steps"] += 1
            self.stats["mixed_rows"] += sum(n for _, n in chunks) + len(dec)
            self.stats["prefill_calls"] += 1
            self.stats["prefill_rows"] += sum(n for _, n in chunks)
            for g, n in chunks:
                g.done += n
            for g in last:
                self.prefilling.remove(g)
                self._start(g, events, prefilled=True)
        else:
            # today's sequence: whole prompts as a group (one batched call, retried one by one), chunks by seq_prefill, then the
            # decode step; a rejected seq_step touched nothing, so only a culprit ends with an "error" event
            group = [g for g, n in chunks if g.done == 0 and g in last]
            for g, n in chunks:
                if g in group:
                    self.prefilling.remove(g)
                    continue
                try:
                    self.eng.seq_prefill(g.seq, g.suffix[g.done:g.done + n])
                    self.stats["prefill_calls"] += 1
                    self.stats["prefill_rows"] += n
                    g.done += n
                    if g in last:
                        self.prefilling.remove(g)
                        self._start(g, events, prefilled=True)
                except Exception as e:
                    self._fail(g, e, events)
            self._prefill_group(group, events)
            last = [g for g in last if g in self.running]
            if dec:
                self.eng.seq_decode([r.seq for r in dec])
        self.stats["decode_steps"] += len(dec)
        return last

    def _step_chunked(self):
        events = self._admit_chunked()
        if not self.running and not self.prefilling:
            return events
        # decode window of the running sequences, bounded as in step(); the pages the mid-prompt requests were promised stay theirs
        steps, starved, had = self.window, None, bool(self.running)
        for r in self.running:
            steps = min(steps, self.eng.max_new - len(r.gen) - r.fresh, self.eng.max_ctx - 2 - self.eng.seq_pos(r.seq))
        steps = max(steps, 0)
        self._preempt_for(steps)
        if steps > 0 and len(self.running) == 1 and not self.prefilling and self._growth(self.running[0], steps) > self.eng.pages_free():
            starved, steps = self.running[0], 0               # alone and the pool is dry: it ends here ("length")
        if self.prefilling:
            dec = list(self.running) if steps > 0 else []
            started = self._mixed_pass(dec, events)           # the prompt rows + the first step of the window
            steps = steps - 1 if dec else (0 if had else self.window - 1)
            for r in started:                                 # their first token is out: what is left of the window is theirs too
                steps = min(steps, self.eng.max_new - 1, self.eng.max_ctx - 2 - self.eng.seq_pos(r.seq))
            steps = max(steps, 0)
            if steps > 0 and self.running:
                self._preempt_for(steps)
                if len(self.running) == 1 and self._growth(self.running[0], steps) > self.eng.pages_free():
                    steps = 0                                 # (a lone sequence on a dry pool: its next iteration ends it)
        if steps > 0 and self.running:
            ids = [r.seq for r in self.running]
            for _ in range(steps):
                self.eng.seq_decode(ids)
            self.stats["decode_steps"] += steps * len(ids)
        self.stats["iterations"] += 1
        torch.cuda.current_stream().synchronize()
        harvest = [self._harvest(r, r is starved) for r in list(self.running)]
        return events + [ev for ev in harvest if ev is not None]

    @torch.no_grad()
    def step(self):
        if self.chunked:
            return self._step_chunked()
        events = self._admit()
        if not self.running:
            return events
        # decode window, bounded by every sequence's token buffer and by the pool's addressable context
        steps, starved = self.window, None
        for r in self.running:
            steps = min(steps, self.eng.max_new - len(r.gen) - r.fresh, self.eng.max_ctx - 2 - self.eng.seq_pos(r.seq))
        if steps > 0:
            self._preempt_for(steps)
            if len(self.running) == 1 and self._growth(self.running[0], steps) > self.eng.pages_free():
                starved, steps = self.running[0], 0           # alone and the pool is dry: it ends here ("length")
        if steps > 0:
            ids = [r.seq for r in self.running]
            for _ in range(steps):
                self.eng.seq_decode(ids)
            self.stats["decode_steps"] += steps * len(ids)
        self.stats["iterations"] += 1
        torch.cuda.current_stream().synchronize()
        harvest = [self._harvest(r, r is starved) for r in list(self.running)]
        return events + [ev for ev in harvest if ev is not None]
