"""Named scenarios that drive ContinuousBatcher through its public surface on the scripted engine (tests/scripted_engine.py); each
returns a JSON-able record: the engine's call list, the events of every step(), the final stats and side tables, the pool at the end.
tests/golden/scheduler_traces.json holds the records of the commit named in its first key; tests/test_scheduler_traces_cpu.py replays
them.  Surface used: constructor, add, step, abort, has_work, stats, errors, logprobs, cached_tokens, len(running), len(waiting),
len(cache.entries), cache.clear, cache.evictions.

    python -m tests.scheduler_scenarios <commit>      writes the golden file (run it on a checkout of <commit>)"""
import json
import os
import sys
from unittest import mock

import torch

from tests import prefix_ref
from tests.scripted_engine import ScriptedEngine, _emb, _expected, _ids, embed_tokens

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scheduler_traces.json")
SAMPLING = dict(temperature=0.8, top_k=5, top_p=0.9, seed=11)
RULES = dict(repetition_penalty=1.3, presence_penalty=0.0, frequency_penalty=0.5, logprobs=2)


def _digests(rows):
    return prefix_ref.digest_bytes(rows.numpy())


class Run:
    def __init__(self, eng, cache=False, hook=True, **kw):
        from vita_amd.serving import ContinuousBatcher, PrefixCache
        self.eng = eng
        self.bt = ContinuousBatcher(eng, embed_tokens=embed_tokens if hook else None,
                                    prefix_cache=PrefixCache(eng, digests=_digests) if cache else False, **kw)
        self.steps, self.notes, self.raised = [], [], None

    def add(self, rid, ids, n, **kw):
        self.bt.add(rid, _emb(ids), n, **kw)

    def step(self, n=1):
        for _ in range(n):
            try:
                self.steps.append([list(e) for e in self.bt.step()])
            except Exception as e:
                self.raised = [type(e).__name__, str(e)]
                return False
        return True

    def drain(self, limit=2000):
        while self.bt.has_work() and limit > 0 and self.step():
            limit -= 1
        assert limit > 0, "scheduler did not terminate"
        return self

    def one(self, rid, ids, n, **kw):
        """one request alone to its end"""
        self.add(rid, ids, n, **kw)
        return self.drain()

    def note(self, what, value):
        self.notes.append([what, len(self.eng.calls), len(self.steps), value])

    def record(self):
        bt, cache = self.bt, self.bt.cache
        return dict(calls=self.eng.calls, steps=self.steps, stats=dict(bt.stats), raised=self.raised, notes=self.notes,
                    errors={k: [type(e).__name__, str(e)] for k, e in bt.errors.items()},
                    logprobs=dict(bt.logprobs), cached_tokens=dict(bt.cached_tokens),
                    running=len(bt.running), waiting=len(bt.waiting),
                    entries=None if cache is None else len(cache.entries), evictions=None if cache is None else cache.evictions,
                    free=self.eng.pages_free(), refs=list(self.eng.refs), slots=sorted(self.eng.seqs))


def _prompt(n, first):
    return [first] + [(first * 7 + 3 * i) % 90 + 1 for i in range(1, n)]


# ---- admission --------------------------------------------------------------------------------------------------------------------
def fifo_slots_eos_length():
    """two slots, four requests, an eos and a length finish, on an engine WITHOUT seq_prefill_batch"""
    run = Run(ScriptedEngine(64 * 32, 2, batch=False, sharing=False), hook=False, window=1)
    for i, p in enumerate([[1, 2, 3], [4, 5, 6, 7, 8], [9], [10, 11]]):
        run.add(f"r{i}", p, 12 if i != 1 else 4, eos={_expected([9], 12)[5]} if i == 2 else ())
    return run.drain()


def fifo_page_limit():
    """three slots, five pages, three two-page prompts: the third waits for pages (no seq_prefill_batch)"""
    run = Run(ScriptedEngine(64 * 5, 3, batch=False, sharing=False), hook=False, window=1)
    for i in range(3):
        run.add(f"r{i}", _prompt(120, i + 1), 4)
    return run.drain()


def groups_close_at_max_prefill():
    run = Run(ScriptedEngine(64 * 32, 4, max_prefill=256), hook=False, window=1)
    for i, n in enumerate([40, 97, 64, 130, 20]):
        run.add(f"r{i}", _prompt(n, i + 1), 6 + i)
    return run.drain()


def group_counts_promised_pages():
    run = Run(ScriptedEngine(64 * 5, 3), hook=False, window=1)
    for i in range(3):
        run.add(f"r{i}", _prompt(120, i + 1), 4)
    return run.drain()


def rejected_group_is_retried_one_by_one():
    """the group call is rejected; of the retries the second seq_prefill fails: one culprit"""
    run = Run(ScriptedEngine(64 * 8, 3, fail={"seq_prefill_batch": 1, "seq_prefill": 2}), hook=False, window=1)
    run.add("ok1", [1, 2, 3], 5)
    run.add("bad", [13, 2], 5)
    run.add("ok2", [4, 5], 5)
    return run.drain()


# ---- preemption -------------------------------------------------------------------------------------------------------------------
def _two_growing(run, **kw):
    run.add("a", list(range(1, 61)), 90, **kw)
    run.add("b", list(range(20, 80)), 90, **kw)
    return run.drain()


def preemption_recomputes():
    return _two_growing(Run(ScriptedEngine(64 * 4, 2, max_new=100), window=4))


def preemption_reprompt_in_chunks_with_rules():
    """the re-prompt is longer than max_prefill: chunks, the rules armed in front of the last one"""
    return _two_growing(Run(ScriptedEngine(64 * 4, 2, max_new=100, max_prefill=64), window=4), rules=RULES, prompt_ids=[3, 5, 8])


def preemption_keeps_sampling_and_rules():
    """draw0 = tokens already generated; the rules are re-armed with prompt set and outputs"""
    return _two_growing(Run(ScriptedEngine(64 * 4, 2, max_new=100), window=4), sampling=SAMPLING, rules=RULES, prompt_ids=[2, 4])


def preemption_without_embed_hook_raises():
    return _two_growing(Run(ScriptedEngine(64 * 4, 2, max_new=100), hook=False, window=4))


# ---- one request fails while it is set up -----------------------------------------------------------------------------------------
def _open_fails(name, n):
    """warm fills the cache; then ok1, bad (which adopts warm's pages) and ok2 arrive together and call `name` in that order"""
    run = Run(ScriptedEngine(64 * 16, 3, fail={name: n}), cache=True, window=1)
    base = _ids(90, 128)
    run.one("warm", base, 2)
    run.add("ok1", _ids(91, 70), 5, sampling=SAMPLING, rules=RULES, prompt_ids=[1])
    run.add("bad", base + _ids(92, 9), 5, sampling=SAMPLING, rules=RULES, prompt_ids=[2])
    run.add("ok2", _ids(93, 30), 5, sampling=SAMPLING, rules=RULES, prompt_ids=[3])
    return run.drain()


def open_fails_at_seq_alloc():
    return _open_fails("seq_alloc", 3)


def open_fails_at_seq_adopt():
    return _open_fails("seq_adopt", 1)


def open_fails_at_seq_set_sampling():
    return _open_fails("seq_set_sampling", 2)


def open_fails_at_seq_set_logit_rules():
    return _open_fails("seq_set_logit_rules", 2)


def prompt_larger_than_the_pool():
    eng = ScriptedEngine(64 * 4, 2)
    run = Run(eng, hook=False, window=1)
    run.one("small", [1, 2], 3)
    eng.max_ctx = 64 * 8                             # lets add() accept the prompt; the POOL stays four pages
    run.add("huge", list(range(1, 90)) * 4, 3)       # 356 rows: six pages
    run.add("after", [7], 3)
    return run.drain()


def abort_running_and_waiting():
    run = Run(ScriptedEngine(64 * 8, 1), hook=False, window=2)
    run.add("a", [1, 2], 30, rules=RULES, prompt_ids=[1])
    run.add("b", [3], 3)
    run.step()
    run.note("abort a (running)", run.bt.abort("a"))
    run.note("abort nope", run.bt.abort("nope"))
    run.drain()
    run.add("c", [5], 2, rules=RULES)
    run.note("abort c (waiting)", run.bt.abort("c"))
    run.note("has_work", run.bt.has_work())
    return run


# ---- prefix cache on --------------------------------------------------------------------------------------------------------------
def _recorded(cache):
    run = Run(ScriptedEngine(64 * 5, 3, max_new=128), cache=cache, window=2)
    common = _ids(80, 100)
    for i in range(4):
        run.add(f"r{i}", common + _ids(81 + i, 5 * i + 3), 40)
    return run.drain()


def shared_prefix_under_preemption_cache_off():
    return _recorded(False)


def shared_prefix_under_preemption_cache_on():
    return _recorded(True)


def cache_eviction_stream():
    run = Run(ScriptedEngine(64 * 4, 2, max_new=128), cache=True)
    run.one("A", _ids(10, 128), 2)
    run.one("B", _ids(11, 64), 2)
    run.note("entries", len(run.bt.cache.entries))
    run.one("x", _ids(21, 63), 70)
    run.note("entries", len(run.bt.cache.entries))
    return run.one("y", _ids(22, 63), 70)


def cache_admission_keeps_what_it_adopts():
    run = Run(ScriptedEngine(64 * 6, 2), cache=True)
    base = _ids(50, 192)
    run.one("warm", base, 2)
    run.one("other", _ids(51, 128), 2)
    run.note("entries", len(run.bt.cache.entries))
    return run.one("probe", base + _ids(52, 100), 3)


def cache_waiting_request_gives_its_pins_back():
    """r2 hits warm's pages but has to wait for pages while r1 runs and grows"""
    run = Run(ScriptedEngine(64 * 6, 2, max_new=128), cache=True, window=2)
    base = _ids(55, 128)
    run.one("warm", base, 2)
    run.add("r1", _ids(56, 190), 70)
    run.add("r2", base + _ids(57, 150), 4)
    return run.drain()


def cache_abort_registers_and_clear():
    run = Run(ScriptedEngine(64 * 32, 3), cache=True)
    run.one("a", _ids(70, 200), 5)
    run.add("b", _ids(70, 200)[:140] + _ids(71, 30), 50)
    run.step(2)
    run.note("abort b", run.bt.abort("b"))
    run.note("entries, free", [len(run.bt.cache.entries), run.eng.pages_free()])
    run.bt.cache.clear()
    return run


SCENARIOS = [fifo_slots_eos_length, fifo_page_limit, groups_close_at_max_prefill, group_counts_promised_pages,
             rejected_group_is_retried_one_by_one, preemption_recomputes, preemption_reprompt_in_chunks_with_rules,
             preemption_keeps_sampling_and_rules, preemption_without_embed_hook_raises, open_fails_at_seq_alloc,
             open_fails_at_seq_adopt, open_fails_at_seq_set_sampling, open_fails_at_seq_set_logit_rules,
             prompt_larger_than_the_pool, abort_running_and_waiting, shared_prefix_under_preemption_cache_off,
             shared_prefix_under_preemption_cache_on, cache_eviction_stream, cache_admission_keeps_what_it_adopts,
             cache_waiting_request_gives_its_pins_back, cache_abort_registers_and_clear]
NAMES = [f.__name__ for f in SCENARIOS]


def play(name):
    """the record of one scenario, as JSON reads it back (tuples are lists, keys are strings)"""
    sync = type("S", (), {"synchronize": lambda self: None})
    with mock.patch.object(torch.cuda, "current_stream", lambda *a, **k: sync()):
        run = SCENARIOS[NAMES.index(name)]()
    return json.loads(json.dumps(run.record()))


if __name__ == "__main__":
    doc = {"generated_from_commit": sys.argv[1], "scenarios": {name: play(name) for name in NAMES}}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{GOLDEN}: {len(NAMES)} scenarios, {os.path.getsize(GOLDEN)} bytes")
