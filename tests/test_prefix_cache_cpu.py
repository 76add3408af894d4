"""Prefix caching without a GPU: the digest restatement (tests/prefix_ref.py) and its chain, and PrefixCache + ContinuousBatcher
(vita_amd/scheduler.py) over the scripted engine with reference-counted pages (tests/scripted_engine.py).  The engine model keeps what
was WRITTEN in its pages and computes a sequence's next token from what its page table reads back, so a wrong page in a table, a page
evicted while in use or a row written into a shared page shows as a wrong id (or trips the model's own assertion)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import prefix_ref  # noqa: E402
from tests.scripted_engine import ScriptedEngine as RefEngine, _drain, _emb, _expected, _ids, no_cuda_sync  # noqa: E402
from tests.scripted_engine import embed_tokens as _embed_tokens  # noqa: E402


# ---- 1. the digest and the chain ------------------------------------------------------------------------------------------------
def _rows(seed, rows=192, cols=24):
    return np.random.default_rng(seed).standard_normal((rows, cols)).astype(np.float32)


def test_fmix32_is_the_published_finaliser():
    # MurmurHash3 fmix32 test values (x -> fmix32(x)): 0 is a fixed point, the others computed by hand from the definition
    assert int(prefix_ref.fmix32(np.array([0], dtype=np.uint32))[0]) == 0

    def by_hand(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    for v in (1, 0x9E3779B9, 0xFFFFFFFF, 123456789):
        assert int(prefix_ref.fmix32(np.array([v], dtype=np.uint32))[0]) == by_hand(v)


def test_single_bit_flips_change_the_block_and_every_later_key_and_none_earlier():
    x = _rows(0)
    d0, k0 = prefix_ref.digests(x), prefix_ref.keys(x)
    rng = np.random.default_rng(1)
    for _ in range(24):
        r, c, bit = int(rng.integers(64, 128)), int(rng.integers(x.shape[1])), int(rng.integers(32))
        y = x.copy()
        y.view(np.uint32)[r, c] ^= np.uint32(1 << bit)
        d1, k1 = prefix_ref.digests(y), prefix_ref.keys(y)
        assert (d1[0] == d0[0]).all() and (d1[2] == d0[2]).all()
        assert (d1[1] != d0[1]).all(), "every lane is a sum of bijections of the words: one changed word changes each"
        assert k1[0] == k0[0] and k1[1] != k0[1] and k1[2] != k0[2]


def test_row_swap_and_signed_zero_change_the_digest():
    x = _rows(2, rows=64)
    y = x.copy()
    y[[3, 40]] = y[[40, 3]]
    assert (prefix_ref.digests(x) != prefix_ref.digests(y)).any()
    z = np.zeros((64, 8), dtype=np.float32)
    nz = z.copy()
    nz[17, 5] = -0.0
    assert (prefix_ref.digests(z)[0] != prefix_ref.digests(nz)[0]).all()


def test_equal_blocks_have_equal_digests_and_different_keys():
    blk = _rows(3, rows=64)
    x = np.concatenate([blk, _rows(4, rows=64), blk, blk[:10]])
    d, k = prefix_ref.digests(x), prefix_ref.keys(x)
    assert d.shape == (3, 4) and (d[0] == d[2]).all() and (d[0] != d[1]).any()
    assert len(set(k)) == 3
    assert prefix_ref.digests(blk[:63]).shape == (0, 4)


def test_product_chain_is_the_restatement():
    from vita_amd import serving
    x = _rows(5)
    db = prefix_ref.digest_bytes(x)
    assert serving.PREFIX_ROOT_KEY == prefix_ref.ROOT_KEY
    assert serving.chain_keys(db, x.shape[1]) == prefix_ref.chain(db, x.shape[1])
    assert serving.chain_keys(db, x.shape[1] + 1) != prefix_ref.chain(db, x.shape[1])
    assert serving.chain_keys(db[1:], x.shape[1], parent=prefix_ref.chain(db[:1], x.shape[1])[0]) == prefix_ref.chain(db, x.shape[1])[1:]


# ---- 2. PrefixCache and the batcher over the scripted engine ---------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _no_cuda_sync(monkeypatch):
    no_cuda_sync(monkeypatch)


def _digests(rows):
    return prefix_ref.digest_bytes(rows.numpy())


def _batcher(eng, **kw):
    from vita_amd.serving import ContinuousBatcher, PrefixCache
    return ContinuousBatcher(eng, embed_tokens=_embed_tokens, prefix_cache=PrefixCache(eng, digests=_digests), **kw)


def _run(bt, rid, ids, n):
    """one request alone to its end -> (its ids, the hit tokens and prefill rows it added)"""
    h0, r0 = bt.stats["prefix_hit_tokens"], bt.stats["prefill_rows"]
    bt.add(rid, _emb(ids), n)
    got, fin = _drain(bt)
    assert fin[rid] == "length" and got[rid] == _expected(ids, n), rid
    return bt.stats["prefix_hit_tokens"] - h0, bt.stats["prefill_rows"] - r0


@pytest.mark.parametrize("S,pages", [(63, 0), (64, 0), (65, 1), (128, 1), (129, 2)])
def test_hit_lengths_follow_the_S_minus_1_rule(S, pages):
    eng = RefEngine(2048, 4)
    bt = _batcher(eng)
    base = _ids(0, 128)
    assert _run(bt, "warm", base, 3) == (0, 128)
    assert len(bt.cache.entries) == 2                       # both full prompt pages are cached
    prompt = (base + _ids(1, 8))[:S]
    hit, rows = _run(bt, "probe", prompt, 5)
    assert hit == 64 * pages and rows == S - 64 * pages
    assert bt.cached_tokens["probe"] == 64 * pages and bt.stats["prefix_queries"] == 2


def test_requests_of_one_admission_group_do_not_share_but_the_next_one_does():
    eng = RefEngine(4096, 4)
    bt = _batcher(eng)
    common = _ids(2, 130)
    pa, pb, pc = common + _ids(3, 20), common + _ids(4, 31), common + _ids(5, 7)
    bt.add("a", _emb(pa), 4)
    bt.add("b", _emb(pb), 4)
    ev = bt.step()
    assert ("prefill_batch", (0, 1), (150, 161)) in eng.calls and bt.stats["prefix_hit_tokens"] == 0
    assert not set(eng.seq_pages(0)) & set(eng.seq_pages(1))
    bt.add("c", _emb(pc), 4)                                 # arrives while a and b run: adopts a's two pages
    got, fin = _drain(bt)
    for rid, new, *_ in ev:
        got[rid] = new + got.get(rid, [])
    assert got == {"a": _expected(pa, 4), "b": _expected(pb, 4), "c": _expected(pc, 4)}
    assert bt.stats["prefix_hit_tokens"] == 128 and bt.stats["prefill_rows"] == 150 + 161 + 137 - 128
    assert ("adopt", 2, (0, 1)) in eng.calls


def test_registration_at_finish_includes_pages_filled_by_generated_tokens():
    eng = RefEngine(2048, 2)
    bt = _batcher(eng)
    p1 = _ids(6, 100)
    assert _run(bt, "r1", p1, 40) == (0, 100)
    out = _expected(p1, 40)
    assert len(bt.cache.entries) == 2                       # positions 0 .. 138 are written: two full pages, the second by decode steps
    p2 = p1 + out[:-1] + _ids(7, 10)
    assert _run(bt, "r2", p2, 6) == (128, len(p2) - 128)
    # without the embed_tokens hook only prompt pages are registered
    from vita_amd.serving import ContinuousBatcher, PrefixCache
    eng2 = RefEngine(2048, 2)
    bt2 = ContinuousBatcher(eng2, prefix_cache=PrefixCache(eng2, digests=_digests))
    bt2.add("r1", _emb(p1), 40)
    _drain(bt2)
    assert len(bt2.cache.entries) == 1


def _eviction_stream():
    """a pool of four pages; chain A (two blocks, tick 1) and chain B (one block, tick 2) are cached, one page is free.  x and y have
    no full prompt block and grow to three pages each while they decode, so every further page is an eviction."""
    eng = RefEngine(4 * 64, 2, max_new=128)
    bt = _batcher(eng)
    _run(bt, "A", _ids(10, 128), 2)
    _run(bt, "B", _ids(11, 64), 2)
    assert len(bt.cache.entries) == 3 and eng.pages_free() == 1
    a_root, a_leaf, b_root = (e.page for e in sorted(bt.cache.entries.values(), key=lambda e: (e.tick, e.children == 0)))
    _run(bt, "x", _ids(21, 63), 70)                          # 63 + 69 rows: two evictions, then its own two full pages are cached
    x_root, x_leaf = (e.page for e in sorted((e for e in bt.cache.entries.values() if e.tick == 3), key=lambda e: e.children == 0))
    _run(bt, "y", _ids(22, 63), 70)
    released = [c[1][0] for c in eng.calls if c[0] == "release" and len(c[1]) == 1]
    return (a_root, a_leaf, b_root, x_root, x_leaf), released, eng.calls, dict(bt.stats)


def test_eviction_takes_childless_entries_first_then_least_recently_used_and_is_reproducible():
    (a_root, a_leaf, b_root, x_root, x_leaf), released, calls, stats = _eviction_stream()
    # x: A's leaf before A's root (same tick, the root has a child), both before the younger B; y: B, then x's leaf (x's root has a child)
    assert released == [a_leaf, a_root, b_root, x_leaf]
    assert stats["prefix_evictions"] == 4 and stats["preemptions"] == 0     # exactly as many as the demand needed
    _, released2, calls2, stats2 = _eviction_stream()
    assert released2 == released and calls2 == calls and stats2 == stats


def test_cached_pages_are_evicted_before_anybody_is_preempted():
    eng = RefEngine(8 * 64, 2, max_new=128)
    bt = _batcher(eng)
    for i in range(3):                                       # fills the cache: 2 + 2 + 2 pages of 8
        _run(bt, f"w{i}", _ids(30 + i, 128), 2)
    assert len(bt.cache.entries) == 6 and eng.pages_free() == 2
    ps = {f"r{i}": _ids(40 + i, 70) for i in range(2)}       # each grows from 2 to 3 pages while it runs: 6 of the 8 pages
    for rid, p in ps.items():
        bt.add(rid, _emb(p), 70)
    got, fin = _drain(bt)
    assert got == {rid: _expected(p, 70) for rid, p in ps.items()}
    assert bt.stats["preemptions"] == 0 and bt.stats["prefix_evictions"] > 0
    assert bt.cache.evictions == bt.stats["prefix_evictions"]


def test_admission_never_evicts_the_pages_it_is_about_to_adopt():
    eng = RefEngine(6 * 64, 2)
    bt = _batcher(eng)
    base = _ids(50, 192)
    _run(bt, "warm", base, 2)                                # pages 0, 1, 2 cached
    _run(bt, "other", _ids(51, 128), 2)                      # two more; one page free
    assert len(bt.cache.entries) == 5 and eng.pages_free() == 1
    # the probe hits the three OLDEST entries and needs 5 - 3 + 0 = 2 pages: one eviction, which must take the other chain's leaf
    p = base + _ids(52, 100)
    n_calls = len(eng.calls)
    warm_pages = [bt.cache.entries[k].page for k in prefix_ref.keys(_emb(base).numpy())]
    hit, rows = _run(bt, "probe", p, 3)
    assert hit == 192 and rows == 100
    during = eng.calls[n_calls:]
    assert ("adopt", 0, tuple(warm_pages)) in during
    evicted = [c[1][0] for c in during if c[0] == "release" and len(c[1]) == 1]
    assert len(evicted) == 1 and not set(evicted) & set(warm_pages)


def test_a_preempted_request_finds_its_own_pages_again():
    eng = RefEngine(4 * 64, 2, max_new=128)
    bt = _batcher(eng)
    pa, pb = _ids(60, 60), _ids(61, 60)
    bt.add("a", _emb(pa), 80)
    bt.add("b", _emb(pb), 80)
    got, fin = _drain(bt)
    assert got == {"a": _expected(pa, 80), "b": _expected(pb, 80)}
    assert bt.stats["preemptions"] >= 1 and bt.stats["prefix_hit_tokens"] >= 64


def test_drain_and_clear_leave_the_pool_whole_and_abort_registers():
    eng = RefEngine(2048, 3)
    bt = _batcher(eng)
    _run(bt, "a", _ids(70, 200), 5)
    bt.add("b", _emb(_ids(70, 200)[:140] + _ids(71, 30)), 50)
    bt.step()
    bt.step()
    assert bt.abort("b") and not bt.has_work()
    assert eng.pages_free() == 32 - len(bt.cache.entries) and len(bt.cache.entries) >= 3
    bt.cache.clear()
    assert eng.pages_free() == 32 and all(r == 0 for r in eng.refs) and not bt.cache.entries


def _recorded(**kw):
    from vita_amd.serving import ContinuousBatcher
    eng = RefEngine(5 * 64, 3, max_new=128)
    bt = ContinuousBatcher(eng, embed_tokens=_embed_tokens, window=2, **kw)
    common = _ids(80, 100)
    for i in range(4):
        bt.add(f"r{i}", _emb(common + _ids(81 + i, 5 * i + 3)), 40)
    got, fin = _drain(bt)
    assert bt.stats["preemptions"] >= 1
    return eng.calls, got, {k: v for k, v in bt.stats.items() if not k.startswith("prefix_") and k != "prefill_rows"}


def test_with_the_cache_off_the_batcher_makes_exactly_the_calls_it_made_without_the_argument():
    calls0, got0, stats0 = _recorded()
    calls1, got1, stats1 = _recorded(prefix_cache=False)
    assert calls0 == calls1 and got0 == got1 and stats0 == stats1
    assert not [c for c in calls0 if c[0] in ("hold", "release", "adopt")]
    # ... and they are the calls of the batcher before the cache existed: alloc / prefill(_batch) / decode / free only, each prompt
    # prefilled whole
    rows = sum(sum(c[2]) if c[0] == "prefill_batch" else c[2] for c in calls0 if c[0].startswith("prefill"))
    assert rows >= 4 * 100


def test_public_switches_exist_and_default_to_off():
    import inspect
    from vita_amd import serving
    assert serving.AsyncEngineArgs().enable_prefix_caching is False
    assert inspect.signature(serving.LLM.__init__).parameters["enable_prefix_caching"].default is False
    assert inspect.signature(serving.ContinuousBatcher.__init__).parameters["prefix_cache"].default is False
    assert serving.RequestOutput("x", []).num_cached_tokens == 0
    assert callable(serving.AsyncLLMEngine.reset_prefix_cache)
    for k in ("prefix_queries", "prefix_hit_tokens", "prefix_evictions", "prefill_rows"):
        assert serving.ContinuousBatcher(RefEngine(1024, 2)).stats[k] == 0
