"""Prefix caching over the paged KV cache (vLLM's enable_prefix_caching; what the reference gets from vLLM's block tables,
web_demo/vllm_tools/vllm_file/mixtral.py:491-501): the device digest of prompt rows (vh_hash_row_blocks), pages with reference counts
(vh_mixtral_seq_hold_prefix / pages_release / seq_adopt / page_refs) and the scheduler's PrefixCache.

Bar (the project's): every request's greedy ids == the fp32 oracle's for THAT request alone, prefill scores atol 1e-3 — whether its
leading K/V rows were computed for it or adopted from another request's pages.  Every oracle run used here has a top-1 / top-2 margin
of at least 4e-3 (four times the bar) at every compared step; _ref asserts it on the oracle's own scores."""
import asyncio
import os

import numpy as np
import pytest
import torch

from oracle import mixtral as om
from tests import prefix_ref
from tests.util import assert_close, to_np
from vita_amd.checkpoint import pack_mixtral, synth_state_dict
from vita_amd.config import VitaConfig

pytestmark = pytest.mark.gpu

MARGIN = 4e-3
# (weights seed, prompt seed) of every scenario: searched on the CPU with the oracle alone for runs whose margin holds (_ref)
SEEDS = {"share": (1, 101), "share_flash": (2, 107), "contract": (3, 100), "batcher": (5, 101), "full": (7, 100), "turns": (9, 103),
         "pressure": (11, 182), "preempt": (13, 101)}


def _model(seed, flash=False):
    """the tiny text geometry of tests/test_paged_gpu.py (H 256, 2 layers) or its 4 : 1-head H 512 one (flash)"""
    from vita_amd.config import TextConfig
    cfg = VitaConfig.tiny()
    if flash:
        cfg.text = TextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2, intermediate_size=1024,
                              num_local_experts=8, vocab_size=2000)
    sd = synth_state_dict(cfg, seed=seed, parts=("text",))
    return cfg, sd, om.MixtralOracle(sd, cfg.text)


def _ref(orc, emb, n_new):
    """the oracle's greedy ids and scores of a request alone; the margin the comparison relies on is asserted here"""
    ids, lg = orc.greedy(emb, n_new)
    top = np.partition(lg, -2, axis=1)[:, -2:]
    margin = float((top[:, 1] - top[:, 0]).min())
    assert margin >= MARGIN, f"oracle margin {margin:.2e} below {MARGIN}: pick another seed"
    return ids, lg


def _rows(sd, cfg, rng, n):
    ids = rng.integers(3, cfg.text.vocab_size, size=n)
    return sd["model.embed_tokens.weight"][ids]


def _engine(cfg, sd, dev, pool=1024, max_prefill=256, max_new=48, max_seqs=4):
    from vita_amd.engine import MixtralEngine
    return MixtralEngine(cfg, pack_mixtral(sd, cfg, dev), dev, max_ctx=pool, max_prefill=max_prefill, max_new=max_new, max_seqs=max_seqs)


def _ids(eng, s, n):
    torch.cuda.synchronize()
    eng.check_device_flag(eng.seq_counters(s).tolist())
    return eng.seq_tokens(s)[:n].tolist()


def _dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _drain(bt, limit=10000):
    got, fin = {}, {}
    for _ in range(limit):
        if not bt.has_work():
            return got, fin
        for rid, new, finished, reason in bt.step():
            got.setdefault(rid, []).extend(new)
            if finished:
                fin[rid] = reason
    raise AssertionError("scheduler did not terminate")


# ---- 1. the digest kernel -----------------------------------------------------------------------------------------------------------
def _hash(x, guard=2):
    """digests of x through the operator, with `guard` sentinel rows behind the output that must stay untouched"""
    from vita_amd import ops
    n = x.shape[0] // 64
    buf = torch.full((n + guard, 4), 0x5A5A5A5A, dtype=torch.int32, device=x.device)
    ops.hash_row_blocks(x, out=buf)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[n:] == 0x5A5A5A5A).all(), "vh_hash_row_blocks wrote behind its output"
    return host[:n].view(np.uint32)


@pytest.mark.parametrize("rows,cols", [(63, 256), (64, 256), (65, 256), (200, 256), (128, 4096), (130, 30)])
def test_hash_row_blocks_is_the_restatement_bit_for_bit(dev, rows, cols):
    """complete blocks only (63 rows: VH_OK, nothing written), several blocks, the released width, and a width that is no multiple
    of four (the kernel's scalar-load form)"""
    g = torch.Generator(device="cpu").manual_seed(rows * 7 + cols)
    x = torch.randn((rows, cols), generator=g).to(dev)
    got = _hash(x)
    want = prefix_ref.digests(x.cpu().numpy())
    assert got.shape == want.shape == (rows // 64, 4)
    assert np.array_equal(got, want)
    assert np.array_equal(_hash(x), got), "the same input gave another digest"


def test_hash_row_blocks_strided_view_and_planted_bit_patterns(dev):
    g = torch.Generator(device="cpu").manual_seed(5)
    big = torch.randn((210, 320), generator=g).to(dev)
    x = big[7:207, :256]                                       # 200 rows from row 7 of a wider tensor: ldx = 320
    assert x.stride(0) == 320 and not x.is_contiguous()
    want = prefix_ref.digests(x.cpu().numpy())
    assert np.array_equal(_hash(x), want)
    assert np.array_equal(_hash(x.contiguous()), want), "the digest depends on ldx or the address"
    # the block's index does not enter: block 1 moved to the front has block 1's digest
    assert np.array_equal(_hash(x[64:128])[0], want[1])
    # -0.0 against 0.0, and a NaN payload, are honoured as bit patterns
    y = x.contiguous().clone()
    y[70, 9] = 0.0
    z = y.clone()
    z[70, 9] = -0.0
    n1, n2 = y.clone(), y.clone()
    n1.view(torch.int32)[130, 200] = 0x7FC00001
    n2.view(torch.int32)[130, 200] = 0x7FC12345
    outs = [_hash(t) for t in (y, z, n1, n2)]
    for t, o in zip((y, z, n1, n2), outs):
        assert np.array_equal(o, prefix_ref.digests(t.cpu().numpy()))
    assert (outs[0][1] != outs[1][1]).all() and (outs[2][2] != outs[3][2]).all()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[2][:2], outs[3][:2])


# ---- 2. engine level: share three pages, diverge ------------------------------------------------------------------------------------
@pytest.mark.parametrize("flash", [False, True])
def test_two_sequences_share_a_prefix_and_diverge(dev, flash):
    """A (200 rows) in slot a; its first three pages are held; slot b adopts them and prefills only B's rows 192.. (B = A[:192] + 40
    other rows).  Both then decode in batched iterations, b across the page boundary at 256; a is freed, a third sequence takes every
    free page, b goes on.  flash: the 4 : 1 head grouping with the flash-form prefill attention forced (k_attn_fa through the page
    table at q_off = 192)."""
    from vita_amd import _lib
    _lib.tune("attn_fa", 2 if flash else 1)
    try:
        _share_and_diverge(dev, flash)
    finally:
        _lib.tune("attn_fa", 1)


def _share_and_diverge(dev, flash):
    joint, alone = 26, 7
    n_new = 1 + joint + alone
    ws, ps = SEEDS["share_flash" if flash else "share"]
    cfg, sd, orc = _model(ws, flash)
    rng = np.random.default_rng(ps)
    A = _rows(sd, cfg, rng, 200)
    B = np.concatenate([A[:192], _rows(sd, cfg, rng, 40)])
    Cq = _rows(sd, cfg, rng, 11 * 64 - 10)                     # the third sequence: every page that is free once a is gone
    refA, refB, refC = _ref(orc, A, 1 + joint), _ref(orc, B, n_new), _ref(orc, Cq, 1 + alone)
    eng = _engine(cfg, sd, dev, pool=1024, max_prefill=704, max_new=n_new + 4)
    pool = eng.pages_free()
    assert pool == 16
    a = eng.seq_alloc()
    eng.seq_prefill(a, _dev(A, dev))
    held = eng.seq_hold_prefix(a, 3)
    assert held == eng.seq_pages(a)[:3] and [eng.page_refs(p) for p in held] == [2, 2, 2]
    b = eng.seq_alloc()
    eng.seq_adopt(b, held)
    assert eng.seq_pos(b) == 192 and eng.seq_pages(b) == held
    lg = eng.seq_prefill(b, _dev(B[192:], dev), want_logits=True)
    assert_close("B prefill scores (rows 192.. behind three adopted pages)", to_np(lg), refB[1][0], atol=1e-3)
    for _ in range(joint):
        eng.seq_decode([a, b])
    pa, pb = eng.seq_pages(a), eng.seq_pages(b)
    assert pa[:3] == pb[:3] == held and not set(pa[3:]) & set(pb[3:])
    assert len(pa) == 4 and len(pb) == 5 and eng.seq_pos(b) == 232 + joint        # b crossed 256 inside the batched iterations
    assert [eng.page_refs(p) for p in held] == [3, 3, 3]
    assert _ids(eng, a, 1 + joint) == refA[0], "sequence A differs from the oracle"
    assert _ids(eng, b, 1 + joint) == refB[0][:1 + joint], "sequence B differs from the oracle"
    eng.seq_free(a)
    assert [eng.page_refs(p) for p in held] == [2, 2, 2]
    assert eng.pages_free() == pool - 3 - 2                     # a's own page came back, the shared ones did not
    c = eng.seq_alloc()
    eng.seq_prefill(c, _dev(Cq, dev))
    assert eng.pages_free() == 0 and not set(eng.seq_pages(c)) & set(held)
    for _ in range(alone):
        eng.seq_decode([b, c])
    assert _ids(eng, b, n_new) == refB[0], "sequence B differs from the oracle after A left"
    assert _ids(eng, c, 1 + alone) == refC[0], "the newcomer differs from the oracle"
    eng.seq_free(b)
    eng.seq_free(c)
    assert eng.pages_free() == pool - 3 and [eng.page_refs(p) for p in held] == [1, 1, 1]
    eng.pages_release(held)
    assert eng.pages_free() == pool
    # the free list is what seq_free alone leaves: the next sequence gets the held pages back in table order
    d = eng.seq_alloc()
    eng.seq_prefill(d, _dev(A[:130], dev))
    assert eng.seq_pages(d) == held
    eng.close()


# ---- 3. contract errors -------------------------------------------------------------------------------------------------------------
def test_contract_errors_change_nothing(dev):
    from vita_amd._lib import VitaHipError
    cfg, sd, orc = _model(SEEDS["contract"][0])
    rng = np.random.default_rng(SEEDS["contract"][1])
    A = _rows(sd, cfg, rng, 100)
    refA = _ref(orc, A, 4)
    eng = _engine(cfg, sd, dev, pool=512, max_seqs=3)
    n_pages = 512 // 64
    a, c = eng.seq_alloc(), eng.seq_alloc()
    eng.seq_prefill(a, _dev(A, dev))
    held = eng.seq_hold_prefix(a, 1)

    def state():
        return (eng.pages_free(), [eng.seq_pos(s) for s in range(3)], [eng.page_refs(p) for p in range(n_pages)],
                [eng.seq_pages(s) for s in (a, c)])

    s0 = state()
    free_page = next(p for p in range(n_pages) if eng.page_refs(p) == 0)
    assert eng.page_refs(-1) == -1 and eng.page_refs(n_pages) == -1
    bad = [("hold past the position", lambda: eng.seq_hold_prefix(a, 2)),
           ("hold of no page", lambda: eng.seq_hold_prefix(a, 0)),
           ("hold on a free slot", lambda: eng.seq_hold_prefix(2, 1)),
           ("adopt into a sequence with pages", lambda: eng.seq_adopt(a, held)),
           ("adopt a free page", lambda: eng.seq_adopt(c, [free_page])),
           ("adopt a page listed twice", lambda: eng.seq_adopt(c, [held[0], held[0]])),
           ("adopt a bad index", lambda: eng.seq_adopt(c, [n_pages])),
           ("adopt as many pages as the pool has", lambda: eng.seq_adopt(c, list(range(n_pages)))),
           ("release a free page", lambda: eng.pages_release([held[0], free_page])),
           ("release more often than held", lambda: eng.pages_release([held[0]] * 3))]
    for name, call in bad:
        with pytest.raises(VitaHipError):
            call()
        assert state() == s0, name
    for _ in range(3):
        eng.seq_decode([a])
    assert _ids(eng, a, 4) == refA[0]
    eng.seq_free(a)
    eng.seq_free(c)
    assert eng.pages_free() == n_pages - 1
    with pytest.raises(VitaHipError, match="reset_prefix_cache"):     # the contiguous-rows entry points would overwrite the held page
        eng.prefill(_dev(A, dev))
    eng.pages_release(held)
    eng.prefill(_dev(A, dev))
    eng.decode(3)
    torch.cuda.synchronize()
    assert eng.generated() == refA[0]
    # reset drops holds as well as sequences
    eng.reset()
    a = eng.seq_alloc()
    eng.seq_prefill(a, _dev(A, dev))
    eng.seq_hold_prefix(a, 1)
    eng.reset()
    assert eng.pages_free() == n_pages and all(eng.page_refs(p) == 0 for p in range(n_pages))
    eng.close()


# ---- 4. the batcher ------------------------------------------------------------------------------------------------------------------
def _batcher(eng, sd, dev, **kw):
    from vita_amd.serving import ContinuousBatcher
    table = torch.from_numpy(sd["model.embed_tokens.weight"]).to(dev)
    return ContinuousBatcher(eng, embed_tokens=lambda ids: table[ids], **kw)


def test_batcher_reuses_a_common_prefix_across_requests_but_not_inside_a_group(dev):
    n_new = 8
    cfg, sd, orc = _model(SEEDS["batcher"][0])
    rng = np.random.default_rng(SEEDS["batcher"][1])
    common, other = _rows(sd, cfg, rng, 130), _rows(sd, cfg, rng, 130)
    prompts = {"r1": np.concatenate([common, _rows(sd, cfg, rng, 20)]), "r2": np.concatenate([common, _rows(sd, cfg, rng, 31)]),
               "r3": np.concatenate([common, _rows(sd, cfg, rng, 7)]),
               "g1": np.concatenate([other, _rows(sd, cfg, rng, 12)]), "g2": np.concatenate([other, _rows(sd, cfg, rng, 25)])}
    refs = {k: _ref(orc, p, n_new)[0] for k, p in prompts.items()}
    eng = _engine(cfg, sd, dev, pool=2048, max_prefill=512)
    bt = _batcher(eng, sd, dev, prefix_cache=True)
    got = {}
    bt.add("r1", _dev(prompts["r1"], dev), n_new)
    got.update(_drain(bt)[0])
    assert bt.stats["prefix_hit_tokens"] == 0 and eng.pages_free() == 32 - 2      # r1's two full prompt pages outlive seq_free
    # (i) after r1 finished
    bt.add("r2", _dev(prompts["r2"], dev), n_new)
    ev = bt.step()
    assert bt.stats["prefix_hit_tokens"] == 128
    # (ii) r3 arrives while r2 runs
    bt.add("r3", _dev(prompts["r3"], dev), n_new)
    more, _ = _drain(bt)
    for rid, new, *_ in ev:
        more[rid] = new + more.get(rid, [])
    got.update(more)
    assert bt.stats["prefix_hit_tokens"] == 256 and bt.cached_tokens == {"r1": 0, "r2": 128, "r3": 128}
    # (iii) g1 and g2 arrive together: one admission group, no sharing inside it
    rows0 = bt.stats["prefill_rows"]
    bt.add("g1", _dev(prompts["g1"], dev), n_new)
    bt.add("g2", _dev(prompts["g2"], dev), n_new)
    got.update(_drain(bt)[0])
    assert bt.stats["prefix_hit_tokens"] == 256 and bt.stats["prefill_rows"] - rows0 == 142 + 155
    assert rows0 == 150 + (161 - 128) + (137 - 128)
    assert bt.stats["prefix_queries"] == 5 and bt.stats["preemptions"] == 0
    for k in prompts:
        assert got[k] == refs[k], (k, got[k], refs[k])
    bt.cache.clear()
    assert eng.pages_free() == 32
    eng.close()


def test_fully_cached_prompt_prefills_its_last_block(dev):
    """a prompt of exactly 128 rows whose two blocks are cached reuses ONE page: the last row's logits make the first token"""
    n_new = 6
    cfg, sd, orc = _model(SEEDS["full"][0])
    P = _rows(sd, cfg, np.random.default_rng(SEEDS["full"][1]), 128)
    ref = _ref(orc, P, n_new)[0]
    eng = _engine(cfg, sd, dev)
    bt = _batcher(eng, sd, dev, prefix_cache=True)
    for rid in ("first", "again"):
        bt.add(rid, _dev(P, dev), n_new)
        got, _ = _drain(bt)
        assert got[rid] == ref, rid
    assert bt.stats["prefix_hit_tokens"] == 64 and bt.stats["prefill_rows"] == 128 + 64 and len(bt.cache.entries) == 2
    eng.close()


def test_pages_filled_by_generated_tokens_are_found_by_the_follow_up_turn(dev):
    from vita_amd.serving import chain_keys, device_digests
    cfg, sd, orc = _model(SEEDS["turns"][0])
    rng = np.random.default_rng(SEEDS["turns"][1])
    P1 = _rows(sd, cfg, rng, 100)
    ids1 = _ref(orc, P1, 40)[0]
    P2 = np.concatenate([P1, sd["model.embed_tokens.weight"][ids1[:-1]], _rows(sd, cfg, rng, 10)])
    ids2, lg2 = _ref(orc, P2, 8)
    eng = _engine(cfg, sd, dev)
    bt = _batcher(eng, sd, dev, prefix_cache=True)
    bt.add("turn1", _dev(P1, dev), 40)
    assert _drain(bt)[0]["turn1"] == ids1
    assert len(bt.cache.entries) == 2                            # positions 0 .. 138: the second page was completed by decode steps
    bt.add("turn2", _dev(P2, dev), 8)
    assert _drain(bt)[0]["turn2"] == ids2
    assert bt.cached_tokens["turn2"] == 128 and bt.stats["prefill_rows"] == 100 + len(P2) - 128
    # the scores of that suffix prefill, once more by hand on the cached pages
    e2 = _dev(P2, dev)
    pages = bt.cache.match(chain_keys(device_digests(e2), e2.shape[1]), 2)
    assert len(pages) == 2
    s = eng.seq_alloc()
    eng.seq_adopt(s, pages)
    lg = eng.seq_prefill(s, e2[128:], want_logits=True)
    assert_close("turn 2 prefill scores behind a page that decode steps completed", to_np(lg), lg2[0], atol=1e-3)
    eng.seq_free(s)
    bt.cache.clear()
    assert eng.pages_free() == 16
    eng.close()


def _pressure_stream(sd, cfg):
    rng = np.random.default_rng(SEEDS["pressure"][1])
    common = _rows(sd, cfg, rng, 130)
    tails = [20, 31, None, 7, None, 50]
    return [np.concatenate([common, _rows(sd, cfg, rng, t)]) if t else _rows(sd, cfg, rng, 140 + 30 * i) for i, t in enumerate(tails)]


def test_cached_pages_yield_under_pressure_before_anybody_is_preempted(dev):
    n_new = 20
    cfg, sd, orc = _model(SEEDS["pressure"][0])
    prompts = _pressure_stream(sd, cfg)
    refs = [_ref(orc, p, n_new)[0] for p in prompts]
    stats = {}
    for cache in (False, True):
        eng = _engine(cfg, sd, dev, pool=512, max_prefill=320, max_seqs=2)
        bt = _batcher(eng, sd, dev, prefix_cache=cache, window=2)
        for i, p in enumerate(prompts):
            bt.add(i, _dev(p, dev), n_new)
        got, fin = _drain(bt)
        for i, r in enumerate(refs):
            assert got[i] == r and fin[i] == "length", (cache, i, got[i], r)
        if cache:
            assert bt.stats["prefix_evictions"] > 0 and bt.stats["prefix_hit_tokens"] >= 128
            bt.cache.clear()
        assert eng.pages_free() == 8
        stats[cache] = dict(bt.stats)
        eng.close()
    assert stats[True]["preemptions"] <= stats[False]["preemptions"]
    assert stats[True]["prefill_rows"] < stats[False]["prefill_rows"]


def test_a_preempted_request_adopts_its_own_pages_when_it_is_recomputed(dev):
    """the dry-pool scenario of test_paged_gpu (4 pages, two sequences that grow to three pages each) with the cache on: the
    preempted request's written pages stay findable, so its re-prompt prefills fewer rows than it has"""
    n_new = 80
    cfg, sd, orc = _model(SEEDS["preempt"][0])
    rng = np.random.default_rng(SEEDS["preempt"][1])
    prompts = [_rows(sd, cfg, rng, 60), _rows(sd, cfg, rng, 62)]
    refs = [_ref(orc, p, n_new)[0] for p in prompts]
    rows = {}
    for cache in (False, True):
        eng = _engine(cfg, sd, dev, pool=256, max_prefill=160, max_new=n_new + 4, max_seqs=2)
        bt = _batcher(eng, sd, dev, prefix_cache=cache, window=4)
        for i, p in enumerate(prompts):
            bt.add(i, _dev(p, dev), n_new)
        got, _ = _drain(bt)
        assert bt.stats["preemptions"] >= 1
        for i, r in enumerate(refs):
            assert got[i] == r, (cache, i, got[i], r)
        if cache:
            assert bt.stats["prefix_hit_tokens"] >= 64
            bt.cache.clear()
        assert eng.pages_free() == 4
        rows[cache] = (bt.stats["prefill_rows"], bt.stats["preemptions"])
        eng.close()
    assert rows[True][1] <= rows[False][1] and rows[True][0] < rows[False][0]


def test_async_engine_reports_num_cached_tokens_and_resets_the_cache(tmp_path, dev):
    from tests import tiny_ckpt
    from vita_amd._lib import VitaHipError
    from vita_amd.serving import AsyncEngineArgs, AsyncLLMEngine, SamplingParams
    d = str(tmp_path / "ckpt")
    os.makedirs(d)
    tiny_ckpt.write(d, seed=31)
    engine = AsyncLLMEngine.from_engine_args(AsyncEngineArgs(model=d, dtype="float16", max_num_seqs=2, max_new_tokens=16,
                                                             kv_pool_tokens=1024, device="cuda:0", enable_prefix_caching=True))
    assert engine.llm.enable_prefix_caching and engine.batcher.cache is not None
    rng = np.random.default_rng(15)
    base = [1] + rng.integers(3, 380, size=140).tolist()
    prompts = [base, base[:135] + rng.integers(3, 380, size=9).tolist()]
    sp = SamplingParams(temperature=0.01, max_tokens=6, skip_special_tokens=False)

    async def one(i):
        last = None
        async for out in engine.generate({"prompt_token_ids": prompts[i]}, sampling_params=sp, request_id=f"q{i}"):
            last = out
        return last

    outs = [asyncio.run(one(0)), asyncio.run(one(1))]
    assert [o.num_cached_tokens for o in outs] == [0, 128] and all(o.finished for o in outs)
    assert engine.batcher.stats["prefill_rows"] == 141 + (144 - 128)
    eng = engine.llm.model.engine
    pool = eng.max_ctx // 64
    assert eng.pages_free() == pool - 2                             # the two full pages of the common prompt
    with pytest.raises(VitaHipError, match="reset_prefix_cache"):     # the one-at-a-time path is fenced while the cache holds pages
        engine.llm.generate({"prompt_token_ids": prompts[0]}, sampling_params=sp)
    assert engine.reset_prefix_cache()
    assert eng.pages_free() == pool
    engine.shutdown()
    for i, o in enumerate(outs):                                    # the ids of the one-at-a-time LLM.generate, which never shares
        exp = engine.llm.generate({"prompt_token_ids": prompts[i]}, sampling_params=sp)[0].outputs[0]
        assert list(o.outputs[0].token_ids) == list(exp.token_ids), i
