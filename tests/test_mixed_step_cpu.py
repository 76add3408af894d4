"""ContinuousBatcher(chunked_prefill=True) (vita_amd/scheduler.py) on the scripted engine with a seq_step entry: which
engine calls an iteration makes, how a long prompt is spread over iterations, when the rules are armed and the prompt's pages
registered, and what abort, preemption and a failing seq_step do to a request that is mid-prompt — without a GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import prefix_ref  # noqa: E402
from tests.scripted_engine import FakeLLM, ScriptedEngine, _drain, _emb, _expected, _ids, next_token, no_cuda_sync  # noqa: E402
from tests.scripted_engine import embed_tokens as _embed_tokens  # noqa: E402

PREFILLS = ("prefill", "prefill_batch")


class StepEngine(ScriptedEngine):
    """the scripted engine with seq_step: the prompt segments are fed as seq_prefill_batch feeds them, the decode members advance as
    seq_decode advances them, after the whole call was checked.  bad: a first prompt id whose segment makes the call raise."""

    def __init__(self, *a, bad=None, **kw):
        super().__init__(*a, **kw)
        self.bad = bad

    def seq_prefill(self, s, emb):
        if self.bad is not None and int(emb.argmax(dim=1)[0]) == self.bad:
            raise RuntimeError("prefill rejected")
        return super().seq_prefill(s, emb)

    def seq_prefill_batch(self, seqs, embs):
        if self.bad is not None and any(int(e.argmax(dim=1)[0]) == self.bad for e in embs):
            raise RuntimeError("batch rejected: a bad segment")
        return super().seq_prefill_batch(seqs, embs)

    def seq_step(self, pf_seqs, embs, dec_seqs):
        self._script("seq_step")
        lens = [int(e.shape[0]) for e in embs]
        both = list(pf_seqs) + list(dec_seqs)
        if len(set(both)) != len(both) or not both or sum(lens) + len(dec_seqs) > self.max_prefill or any(n < 1 for n in lens):
            raise RuntimeError("step rejected")
        if self.bad is not None and any(int(e.argmax(dim=1)[0]) == self.bad for e in embs):
            raise RuntimeError("step rejected: a bad segment")
        short = sum(self._short(self.seqs[s], n) for s, n in zip(pf_seqs, lens)) + sum(self._short(self.seqs[s], 1) for s in dec_seqs)
        if short > len(self._free):
            raise RuntimeError("KV pool exhausted")
        assert all(self.seqs[s]["toks"] for s in dec_seqs), "a decode member without a token"
        for s, e in zip(pf_seqs, embs):
            self._feed(self.seqs[s], e.argmax(dim=1).tolist())
        for s in dec_seqs:
            q = self.seqs[s]
            self._write(q, [q["toks"][-1]])
            q["toks"].append(next_token(self._hist(q)))
        self.calls.append(("step", tuple(pf_seqs), tuple(lens), tuple(dec_seqs)))


@pytest.fixture(autouse=True)
def _no_cuda_sync(monkeypatch):
    no_cuda_sync(monkeypatch)


def _digests(rows):
    return prefix_ref.digest_bytes(rows.numpy())


def _batcher(eng, budget=128, **kw):
    from vita_amd.serving import ContinuousBatcher
    return ContinuousBatcher(eng, embed_tokens=_embed_tokens, chunked_prefill=True, max_batched_tokens=budget, **kw)


def _drain_after(bt, *first):
    """_drain, with the events of steps already taken in front"""
    got, fin = _drain(bt)
    for ev in reversed(first):
        for rid, new, finished, reason in ev:
            got[rid] = new + got.get(rid, [])
            if finished:
                fin[rid] = reason
    return got, fin


def _iterate(bt, eng, arrivals, limit=2000):
    """step until idle; arrivals: {iteration: [(id, prompt ids, max_tokens)]} -> (tokens per request, finish reasons, per iteration
    (the engine calls it made, its events))"""
    got, fin, its = {}, {}, []
    for it in range(limit):
        for rid, ids, n in arrivals.get(it, ()):
            bt.add(rid, _emb(ids), max_tokens=n)
        if not bt.has_work() and it > max(arrivals):
            return got, fin, its
        n0 = len(eng.calls)
        ev = bt.step()
        its.append((eng.calls[n0:], ev))
        for rid, new, finished, reason in ev:
            got.setdefault(rid, []).extend(new)
            if finished:
                fin[rid] = reason
    raise AssertionError("scheduler did not terminate")


def test_one_seq_step_per_iteration_with_prompt_rows_and_a_long_prompt_in_three_chunks():
    eng = StepEngine(pool_tokens=64 * 32, max_seqs=4, max_new=64)
    bt = _batcher(eng, budget=128, window=1)
    P = {"a": _ids(1, 20), "b": _ids(2, 30), "long": _ids(3, 300), "d": _ids(4, 10)}
    arrivals = {0: [("a", P["a"], 30), ("b", P["b"], 30)], 3: [("long", P["long"], 12)], 5: [("d", P["d"], 8)]}
    got, fin, its = _iterate(bt, eng, arrivals)
    assert got == {k: _expected(P[k], n) for k, n in (("a", 30), ("b", 30), ("long", 12), ("d", 8))}
    assert set(fin.values()) == {"length"} and eng.free == 32 and not eng.seqs
    assert not eng.trace(*PREFILLS), "a prefill call with the flag on"
    mixed = 0
    for calls, ev in its:
        steps = [c for c in calls if c[0] == "step"]
        assert len(steps) <= 1
        for _, pf, lens, dec in steps:
            assert lens and sum(lens) + len(dec) <= 128
            mixed += 1
        if not steps:                    # an iteration without prompt rows is today's: decode calls only
            assert all(c[0] in ("decode", "free", "alloc") for c in calls), calls
    assert mixed == bt.stats["mixed_steps"] and bt.stats["mixed_rows"] == sum(sum(c[2]) + len(c[3]) for c in eng.trace("step"))
    assert bt.stats["prefill_rows"] == 20 + 30 + 300 + 10 and bt.stats["prefills"] == 4
    # the 300-row prompt next to two running requests: 126 + 126 + 48 rows over three consecutive iterations ...
    slot = next(c[1] for c in eng.calls if c[0] == "step" and 126 in c[2])[0]
    chunks = [(i, c) for i, (calls, _) in enumerate(its) for c in calls if c[0] == "step" and slot in c[1] and c[2][c[1].index(slot)] in (126, 48)]
    assert [c[2][c[1].index(slot)] for _, c in chunks] == [126, 126, 48]
    assert [i for i, _ in chunks] == list(range(chunks[0][0], chunks[0][0] + 3))
    # ... in each of which every running request receives exactly one token, and the long one its first with the third
    for k, (i, c) in enumerate(chunks):
        assert len(c[3]) == 2
        ev = {rid: new for rid, new, *_ in its[i][1]}
        assert len(ev["a"]) == 1 and len(ev["b"]) == 1
        assert ("long" in ev) == (k == 2) and (k < 2 or len(ev["long"]) == 1)
    # "d" arrived while the long prompt was mid-prompt: its rows ride behind the long prompt's last chunk
    assert chunks[2][1][2] == (48, 10)


def test_rules_are_armed_once_in_front_of_the_last_chunk_and_draw0_is_unchanged():
    from vita_amd.serving import ContinuousBatcher
    long, short = _ids(5, 300), _ids(6, 12)
    rules = dict(repetition_penalty=1.2, presence_penalty=0.0, frequency_penalty=0.5, logprobs=2)
    samp = dict(temperature=0.7, top_k=5, top_p=0.9, seed=3)
    traces = {}
    for on in (False, True):
        eng = StepEngine(pool_tokens=64 * 32, max_seqs=3, max_new=64)
        bt = _batcher(eng, budget=128) if on else ContinuousBatcher(eng, embed_tokens=_embed_tokens)
        bt.add("s", _emb(short), max_tokens=20)
        bt.add("l", _emb(long), max_tokens=6, sampling=samp, rules=rules, prompt_ids=long)
        got, fin = _drain(bt)
        assert got == {"s": _expected(short, 20), "l": _expected(long, 6)}
        assert [list(d) for d in bt.logprobs["l"]] == [[t + 1, t + 2, t] for t in got["l"]]
        traces[on] = eng
    on, off = traces[True], traces[False]
    assert on.trace("set_sampling") == off.trace("set_sampling") and on.trace("set_sampling")[0][2] == 0
    armed = on.trace("set_logit_rules")
    assert armed == off.trace("set_logit_rules") and len(armed) == 1 and armed[0][2:] == (tuple(long), (), rules)
    steps = [i for i, c in enumerate(on.calls) if c[0] == "step" and armed[0][1] in c[1]]
    assert len(steps) == 3 and steps[1] < on.calls.index(armed[0]) < steps[2]


def test_nothing_is_registered_before_the_last_chunk_and_a_later_identical_prompt_hits():
    from vita_amd.serving import PrefixCache
    eng = StepEngine(pool_tokens=64 * 32, max_seqs=3, max_new=64)
    bt = _batcher(eng, budget=128, prefix_cache=PrefixCache(eng, digests=_digests))
    long = _ids(7, 300)
    bt.add("first", _emb(long), max_tokens=4)
    n_steps = 0
    while bt.has_work() and n_steps < 3:
        n0 = len(eng.calls)
        bt.step()
        new = eng.calls[n0:]
        n_steps += sum(1 for c in new if c[0] == "step")
        if n_steps < 3:
            assert not eng.trace("hold") and not bt.cache.entries, "pages registered before the last chunk was enqueued"
    assert [c[2] for c in eng.trace("step")] == [(128,), (128,), (44,)]
    assert eng.trace("hold") == [("hold", 0, 4)] and len(bt.cache.entries) == 4
    got, fin = _drain(bt)
    bt.add("again", _emb(long), max_tokens=4)
    got2, _ = _drain(bt)
    assert got2["again"] == _expected(long, 4)
    assert bt.cached_tokens["again"] == 256 and bt.stats["prefix_hit_tokens"] == 256
    assert eng.trace("step")[-1][2] == (300 - 256,)


def test_abort_of_a_mid_prompt_request_returns_its_slot_and_pages():
    eng = StepEngine(pool_tokens=64 * 16, max_seqs=2, max_new=64)
    bt = _batcher(eng, budget=128)
    run, long = _ids(8, 10), _ids(9, 300)
    bt.add("run", _emb(run), max_tokens=12)
    bt.step()
    bt.add("long", _emb(long), max_tokens=4)
    bt.step()
    assert [r.id for r in bt.prefilling] == ["long"] and bt.prefilling[0].done == 127 and len(eng.seqs) == 2
    assert bt.abort("long") and not bt.prefilling and len(eng.seqs) == 1 and eng.free == 16 - 1
    got, fin = _drain(bt)
    assert fin == {"run": "length"} and eng.free == 16 and not eng.seqs
    bt.add("long", _emb(long), max_tokens=4)          # and the same prompt is served afterwards, from its first row
    got, fin = _drain(bt)
    assert got["long"] == _expected(long, 4)


def test_a_mid_prompt_request_yields_before_a_running_one_and_requeues_with_its_full_prompt():
    """6 pages: the running request (62 rows: one page, a second at position 64, a third at 128) and a 250-row prompt (4 pages
    promised) that trickles in 3 rows per iteration.  Admission left one page of headroom for the runner; when it needs its third page
    the mid-prompt request (the youngest, nothing produced yet) gives its slot and pages back, waits, and goes in again from row 0."""
    eng = StepEngine(pool_tokens=64 * 6, max_seqs=2, max_new=100)
    bt = _batcher(eng, budget=4)
    run, long = _ids(10, 62), _ids(11, 250)
    bt.add("run", _emb(run), max_tokens=80)
    evs = [bt.step() for _ in range(16)]                # 62 rows, 4 per pass: the 16th carries the last two
    assert not bt.prefilling and [r.id for r in bt.running] == ["run"]
    bt.add("long", _emb(long), max_tokens=3)
    evs.append(bt.step())
    slot = bt.prefilling[0].seq
    assert [r.id for r in bt.prefilling] == ["long"] and bt.prefilling[0].done == 3
    got, fin = _drain_after(bt, *evs)
    assert got == {"run": _expected(run, 80), "long": _expected(long, 3)} and eng.free == 6 and not eng.seqs
    assert bt.stats["preemptions"] == 1 and fin == {"run": "length", "long": "length"}
    cut = eng.calls.index(("free", slot))               # the mid-prompt request's slot goes back while "run" still runs
    before = sum(c[2][c[1].index(slot)] for c in eng.calls[:cut] if c[0] == "step" and slot in c[1])
    assert 0 < before < 250 and any(c[0] == "decode" for c in eng.calls[cut:])
    assert bt.stats["prefill_rows"] == 62 + before + 250 == sum(sum(c[2]) for c in eng.trace("step"))


def test_a_failing_seq_step_falls_back_and_only_the_culprit_fails():
    eng = StepEngine(pool_tokens=64 * 16, max_seqs=3, max_new=64, bad=13)
    bt = _batcher(eng, budget=128)
    ok1, bad, ok2 = _ids(12, 9), [13] + _ids(13, 5), _ids(14, 7)
    bt.add("ok1", _emb(ok1), max_tokens=6)
    ev = bt.step()
    bt.add("bad", _emb(bad), max_tokens=6)
    bt.add("ok2", _emb(ok2), max_tokens=6)
    got, fin = _drain_after(bt, ev)
    assert fin == {"ok1": "length", "bad": "error", "ok2": "length"}
    assert got["ok1"] == _expected(ok1, 6) and got["ok2"] == _expected(ok2, 6) and got.get("bad", []) == []
    assert isinstance(bt.errors.pop("bad"), RuntimeError) and bt.stats["failed"] == 1
    assert eng.free == 16 and not eng.seqs
    assert eng.trace("prefill", "prefill_batch"), "the fallback did not go through today's prefill calls"


def test_engine_without_seq_step_makes_todays_calls():
    from vita_amd.serving import ContinuousBatcher
    prompts = {"a": _ids(15, 40), "b": _ids(16, 97), "c": _ids(17, 64)}
    calls = []
    for kw in (dict(), dict(chunked_prefill=True, max_batched_tokens=128)):
        eng = ScriptedEngine(pool_tokens=64 * 16, max_seqs=3, max_new=64, max_prefill=256)
        bt = ContinuousBatcher(eng, **kw)
        assert not bt.chunked
        for k, p in prompts.items():
            bt.add(k, _emb(p), max_tokens=5)
        got, _ = _drain(bt)
        assert got == {k: _expected(p, 5) for k, p in prompts.items()}
        calls.append(eng.calls)
    assert calls[0] == calls[1] and any(c[0] == "prefill_batch" for c in calls[0])


def test_budget_limits():
    from vita_amd.serving import ContinuousBatcher
    eng = StepEngine(pool_tokens=64 * 16, max_seqs=3, max_prefill=256)
    assert ContinuousBatcher(eng, chunked_prefill=True).budget == 256
    assert ContinuousBatcher(eng).chunked is False and "mixed_steps" not in ContinuousBatcher(eng).stats
    with pytest.raises(ValueError):
        ContinuousBatcher(eng, chunked_prefill=True, max_batched_tokens=257)
    with pytest.raises(ValueError):
        ContinuousBatcher(eng, chunked_prefill=True, max_batched_tokens=3)      # no prompt row next to three running sequences


def test_engine_args_reach_the_batcher(monkeypatch):
    import inspect
    from vita_amd import serving
    assert serving.AsyncEngineArgs().enable_chunked_prefill is False and serving.AsyncEngineArgs().max_num_batched_tokens is None
    assert inspect.signature(serving.LLM.__init__).parameters["enable_chunked_prefill"].default is False
    assert inspect.signature(serving.ContinuousBatcher.__init__).parameters["chunked_prefill"].default is False

    class StepLLM(FakeLLM):
        def __init__(self, *a, enable_chunked_prefill=False, max_num_batched_tokens=None, **kw):
            super().__init__()
            self.model.engine = StepEngine(64 * 16, 3, max_new=64)
            self.enable_chunked_prefill, self.max_num_batched_tokens = enable_chunked_prefill, max_num_batched_tokens

    monkeypatch.setattr(serving, "LLM", StepLLM)
    engine = serving.AsyncLLMEngine.from_engine_args(serving.AsyncEngineArgs(model="/nonexistent", enable_chunked_prefill=True,
                                                                             max_num_batched_tokens=128, max_num_seqs=3))
    try:
        assert engine.batcher.chunked and engine.batcher.budget == 128

        async def one():
            last = None
            async for out in engine.generate({"prompt_token_ids": _ids(18, 200)}, serving.SamplingParams(max_tokens=5), request_id="r"):
                last = out
            return list(last.outputs[0].token_ids)

        import asyncio
        assert asyncio.run(one()) == _expected(_ids(18, 200), 5)
        assert [c[2] for c in engine.llm.model.engine.trace("step")] == [(128,), (72,)]
    finally:
        engine.shutdown()
    off = serving.AsyncLLMEngine(StepLLM(), max_num_seqs=3)
    try:
        assert not off.batcher.chunked
    finally:
        off.shutdown()
