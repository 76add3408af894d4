"""ContinuousBatcher's grouped prefill (vita_amd/scheduler.py) on the scripted engine, without a GPU: the admitted requests of a step
are prefilled in groups of up to max_prefill rows, a group of two or more through ONE seq_prefill_batch call; admission itself
(FIFO order, slot and page rules) is what it was, with the pages promised to a group counted until its call has run.  The engine
model is tests/scripted_engine.py's (a sequence's next token is a pure function of the tokens it has consumed), whose
seq_prefill_batch checks the whole call before it touches anything, as the C entry point does."""
import ctypes as C

import pytest
import torch

from tests.scripted_engine import ScriptedEngine, _drain, _emb, _expected, no_cuda_sync


class BatchEngine(ScriptedEngine):
    """with seq_prefill_batch, without the shared-page entries"""

    def __init__(self, *a, **kw):
        super().__init__(*a, sharing=False, **kw)


def _prefills(eng):
    return eng.trace("prefill", "prefill_batch", "rejected")


@pytest.fixture(autouse=True)
def _no_cuda_sync(monkeypatch):
    no_cuda_sync(monkeypatch)


def _drain_after(first_events, bt):
    """_drain, with the events of a step the test already took"""
    got, fin = _drain(bt)
    for rid, new, finished, reason in reversed(first_events):
        got[rid] = list(new) + got.get(rid, [])
        if finished:
            fin[rid] = reason
    return got, fin


def _prompt(n, first):
    return [first] + [(first * 7 + 3 * i) % 90 + 1 for i in range(1, n)]


def test_admitted_requests_are_prefilled_in_groups():
    from vita_amd.serving import ContinuousBatcher
    eng = BatchEngine(pool_tokens=64 * 64, max_seqs=4, max_prefill=256)
    bt = ContinuousBatcher(eng, window=1)
    lens = [40, 97, 64, 130, 20]
    prompts = [_prompt(n, i + 1) for i, n in enumerate(lens)]
    for i, p in enumerate(prompts):
        bt.add(i, _emb(p), max_tokens=6 + i)
    ev = bt.step()
    first = _prefills(eng)
    # four slots: four requests admitted in the first step, (40, 97, 64) in ONE call (201 rows; 130 more would pass 256), 130 alone
    assert first == [("prefill_batch", (0, 1, 2), (40, 97, 64)), ("prefill", 3, 130)], first
    assert bt.stats["prefills"] == 4 and bt.stats["prefill_calls"] == 2 and len(bt.running) == 4
    got, fin = _drain_after(ev, bt)
    for i, p in enumerate(prompts):
        assert got[i] == _expected(p, 6 + i), i
    assert bt.stats["prefills"] == 5 and bt.stats["prefill_calls"] == 3 and bt.stats["failed"] == 0
    assert _prefills(eng)[2][0] == "prefill" and eng.free == 64 and not eng.seqs


def test_pages_promised_to_the_group_are_counted():
    """each prompt fits the pool alone, the three together do not: the third waits for pages instead of sinking the group call."""
    from vita_amd.serving import ContinuousBatcher
    eng = BatchEngine(pool_tokens=64 * 5, max_seqs=3, max_prefill=512)
    bt = ContinuousBatcher(eng, window=1)
    prompts = [_prompt(120, i + 1) for i in range(3)]                     # two pages each
    for i, p in enumerate(prompts):
        bt.add(i, _emb(p), max_tokens=4)
    ev = bt.step()
    assert _prefills(eng) == [("prefill_batch", (0, 1), (120, 120))]
    assert len(bt.running) == 2 and len(bt.waiting) == 1 and not any(e[3] == "error" for e in ev)
    got, fin = _drain_after(ev, bt)
    assert fin == {0: "length", 1: "length", 2: "length"} and bt.stats["failed"] == 0
    for i, p in enumerate(prompts):
        assert got[i] == _expected(p, 4), i
    assert eng.free == 5 and not eng.seqs


def test_a_rejected_group_is_retried_request_by_request():
    from vita_amd.serving import ContinuousBatcher

    class Flaky(BatchEngine):
        def seq_prefill_batch(self, seqs, embs):
            if any(int(e.argmax(dim=1)[0]) == 13 for e in embs):         # the whole call is refused before it touches anything
                self.calls.append(("rejected", tuple(seqs)))
                raise RuntimeError("batch rejected")
            return super().seq_prefill_batch(seqs, embs)

        def seq_prefill(self, s, emb):
            if int(emb.argmax(dim=1)[0]) == 13:
                raise RuntimeError("prefill rejected")
            return super().seq_prefill(s, emb)

    eng = Flaky(pool_tokens=64 * 8, max_seqs=3)
    bt = ContinuousBatcher(eng, window=1)
    bt.add("ok1", _emb([1, 2, 3]), max_tokens=5)
    bt.add("bad", _emb([13, 2]), max_tokens=5)
    bt.add("ok2", _emb([4, 5]), max_tokens=5)
    events = []
    for _ in range(100):
        if not bt.has_work():
            break
        events += bt.step()
    fin = {e[0]: e[3] for e in events if e[2]}
    got = {}
    for rid, new, _, _ in events:
        got.setdefault(rid, []).extend(new)
    assert fin == {"ok1": "length", "bad": "error", "ok2": "length"}
    assert sum(1 for e in events if e[3] == "error") == 1
    assert got["ok1"] == _expected([1, 2, 3], 5) and got["ok2"] == _expected([4, 5], 5) and got["bad"] == []
    assert _prefills(eng)[:3] == [("rejected", (0, 1, 2)), ("prefill", 0, 3), ("prefill", 2, 2)], _prefills(eng)[:3]
    assert isinstance(bt.errors.pop("bad"), RuntimeError) and bt.stats["failed"] == 1 and bt.stats["prefills"] == 2
    assert eng.free == 8 and not eng.seqs


def test_recompute_longer_than_max_prefill_still_goes_in_chunks():
    from vita_amd.serving import ContinuousBatcher
    eng = BatchEngine(pool_tokens=64 * 4, max_seqs=2, max_new=100, max_prefill=64)
    table = torch.eye(ScriptedEngine.V)
    bt = ContinuousBatcher(eng, embed_tokens=lambda ids: table[ids], window=4)
    pa, pb = list(range(1, 61)), list(range(20, 82))[:60]
    bt.add("a", _emb(pa), max_tokens=90)
    bt.add("b", _emb(pb), max_tokens=90)
    got, fin = _drain(bt)
    assert bt.stats["preemptions"] >= 1 and bt.stats["failed"] == 0
    assert got["a"] == _expected(pa, 90) and got["b"] == _expected(pb, 90)       # the re-prompt (> 64 rows) continued exactly
    assert all(c[2] <= 64 for c in eng.calls if c[0] == "prefill")
    assert all(sum(c[2]) <= 64 for c in eng.calls if c[0] == "prefill_batch")
    assert any(c[0] == "prefill" and c[2] < 64 for c in eng.calls)               # a chunk tail: the chunked path ran
    assert eng.free == 4 and fin == {"a": "length", "b": "length"}


def test_c_entry_point_rejects_a_null_engine():
    from vita_amd import _lib
    lib = _lib.load()
    ids, lens = (C.c_int * 2)(0, 1), (C.c_int * 2)(3, 4)
    assert lib.vh_mixtral_seq_prefill_batch(None, ids, lens, 2, None, None, None) != 0
    assert b"vh_mixtral_seq_prefill_batch" in lib.vh_last_error()
    with pytest.raises(_lib.VitaHipError, match="null pointer"):
        _lib.check(lib.vh_mixtral_seq_prefill_batch(None, ids, lens, 2, None, None, None), "vh_mixtral_seq_prefill_batch")
