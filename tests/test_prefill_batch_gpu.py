"""vh_mixtral_seq_prefill_batch: the prompts of several admitted requests in ONE pass over the weights — everything
row-wise runs on the rows of all segments at once, RoPE + KV write and causal paged attention take the segment descriptors, the
first tokens come from the batched head with each sequence's own sampling.

Bar (tests/test_paged_gpu.py's): every sequence's ids equal the fp32 oracle's ids for THAT sequence alone, prefill scores within
1e-3 — not bit-identity with the one-by-one path (the K split of the projections follows the tile count of the pass)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import mixtral as om
from tests import q8_ref
from tests import sampling_ref
from tests.util import assert_close, to_np
from vita_amd.checkpoint import pack_mixtral, synth_state_dict
from vita_amd.config import TextConfig, VitaConfig

pytestmark = pytest.mark.gpu

MIXED = [40, 97, 64, 130, 20, 75]
FLASH_TEXT = dict(hidden_size=512, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2, intermediate_size=1024,
                  num_local_experts=8, vocab_size=2000)       # the released 4 : 1 head grouping: the flash kernel's


def _setup(dev, lens, n_new, seed=0, pool=2048, max_seqs=6, max_prefill=None, text=None, experts=None, oracle_sd=None):
    from vita_amd.engine import MixtralEngine
    cfg = VitaConfig.tiny()
    if text is not None:
        cfg.text = TextConfig(**text)
    sd = synth_state_dict(cfg, seed=seed, parts=("text",))
    rng = np.random.default_rng(seed + 7)
    orc = om.MixtralOracle(oracle_sd(sd) if oracle_sd else sd, cfg.text)
    reqs = []
    for S in lens:
        ids_in = rng.integers(3, cfg.text.vocab_size, size=S)
        emb = sd["model.embed_tokens.weight"][ids_in]
        orc.reset()
        ref_ids, ref_lg = orc.greedy(emb, n_new)
        reqs.append(dict(emb=torch.from_numpy(emb).to(dev), ref_ids=ref_ids, ref_lg=ref_lg))
    packed = pack_mixtral(sd, cfg, dev, experts=experts) if experts else pack_mixtral(sd, cfg, dev)
    eng = MixtralEngine(cfg, packed, dev, max_ctx=pool, max_prefill=max_prefill or sum(lens), max_new=n_new + 4, max_seqs=max_seqs)
    return cfg, sd, eng, reqs


def _ids(eng, s, n):
    torch.cuda.synchronize()
    eng.check_device_flag(eng.seq_counters(s).tolist())
    return eng.seq_tokens(s)[:n].tolist()


def _one_pass_then_decode(eng, reqs, n_new):
    """all requests in ONE call, scores of every segment's last row, then n_new - 1 batched decode iterations"""
    total = eng.pages_free()
    seqs = [eng.seq_alloc() for _ in reqs]
    lg = eng.seq_prefill_batch(seqs, [r["emb"] for r in reqs], want_logits=True)
    assert tuple(lg.shape) == (len(reqs), eng.c.vocab)
    for i, r in enumerate(reqs):
        assert_close(f"segment {i} prefill scores", to_np(lg[i]), r["ref_lg"][0], atol=1e-3)
        assert eng.seq_pos(seqs[i]) == r["emb"].shape[0]
    for _ in range(n_new - 1):
        eng.seq_decode(seqs)
    for i, r in enumerate(reqs):
        assert _ids(eng, seqs[i], n_new) == r["ref_ids"], f"sequence {i} differs from its oracle"
        assert eng.seq_pos(seqs[i]) == r["emb"].shape[0] + n_new - 1
    for s in seqs:
        eng.seq_free(s)
    assert eng.pages_free() == total


@pytest.mark.parametrize("flash", [False, True])
def test_six_prompts_in_one_pass_match_their_oracles(dev, flash):
    """the mixed list in one call (426 rows), then 13 batched decode iterations.  flash: the 4 : 1 head grouping with the flash
    kernel forced — its segmented instantiation (k_attn_fa<3>), one launch per layer for all six segments."""
    from vita_amd import _lib
    n_new = 14
    _lib.tune("attn_fa", 2 if flash else 1)
    try:
        _, _, eng, reqs = _setup(dev, MIXED, n_new, seed=11, text=FLASH_TEXT if flash else None)
        _one_pass_then_decode(eng, reqs, n_new)
        eng.close()
    finally:
        _lib.tune("attn_fa", 1)


@pytest.mark.parametrize("flash", [False, True])
def test_interleaved_pages_and_a_later_chunk(dev, flash):
    """A's first 60 rows by seq_prefill, two unrelated sequences take pages in between, then ONE call with A's remaining rows (at
    position 60: its keys start in a page written earlier), and B's and C's whole prompts."""
    from vita_amd import _lib
    n_new = 10
    _lib.tune("attn_fa", 2 if flash else 1)
    try:
        _, _, eng, (A, B, Cq, X, Y) = _setup(dev, [150, 70, 33, 65, 20], n_new, seed=4, max_prefill=256,
                                             text=FLASH_TEXT if flash else None)
        a = eng.seq_alloc()
        eng.seq_prefill(a, A["emb"][:60])
        x, y = eng.seq_alloc(), eng.seq_alloc()
        eng.seq_prefill(x, X["emb"])
        eng.seq_prefill(y, Y["emb"])
        b, c = eng.seq_alloc(), eng.seq_alloc()
        lg = eng.seq_prefill_batch([a, b, c], [A["emb"][60:], B["emb"], Cq["emb"]], want_logits=True)
        pa = eng.seq_pages(a)
        assert len(pa) == 3 and pa[1] != pa[0] + 1, pa            # A's later pages lie behind X's and Y's
        assert [eng.seq_pos(s) for s in (a, b, c)] == [150, 70, 33]
        for i, r in enumerate((A, B, Cq)):
            assert_close(f"segment {i} scores", to_np(lg[i]), r["ref_lg"][0], atol=1e-3)
        for _ in range(n_new - 1):
            eng.seq_decode([a, b, c, x, y])
        for name, s, r in (("A", a, A), ("B", b, B), ("C", c, Cq), ("X", x, X), ("Y", y, Y)):
            assert _ids(eng, s, n_new) == r["ref_ids"], f"sequence {name} differs from its oracle"
        eng.close()
    finally:
        _lib.tune("attn_fa", 1)


def test_one_segment_is_seq_prefill_bit_for_bit(dev):
    outs = []
    for batch in (False, True):
        _, _, eng, (A,) = _setup(dev, [97], 2, seed=2, max_seqs=2)
        s = eng.seq_alloc()
        lg = eng.seq_prefill_batch([s], [A["emb"]], want_logits=True)[0] if batch else eng.seq_prefill(s, A["emb"], want_logits=True)
        eng.seq_decode([s])
        outs.append((_ids(eng, s, 2), lg.clone(), eng.seq_pos(s)))
        assert outs[-1][0] == A["ref_ids"]
        eng.close()
    assert outs[0][0] == outs[1][0] and outs[0][2] == outs[1][2] and torch.equal(outs[0][1], outs[1][1])


def test_each_segment_draws_with_its_own_sampling(dev):
    """greedy, temperature only, top-k + top-p, temperature only with another seed — in one call: the first token of a segment is
    the contract's draw (tests/sampling_ref.py) from THAT segment's returned scores at draw index 0."""
    n_new = 6
    _, _, eng, reqs = _setup(dev, [40, 97, 64, 20], n_new, seed=6, max_seqs=4)
    params = [None, dict(temperature=0.8, seed=1), dict(temperature=0.9, top_k=20, top_p=0.9, seed=2), dict(temperature=1.3, seed=3)]
    seqs = [eng.seq_alloc() for _ in reqs]
    for s, p in zip(seqs, params):
        if p is not None:
            eng.seq_set_sampling(s, **p)
    lg = eng.seq_prefill_batch(seqs, [r["emb"] for r in reqs], want_logits=True)
    for _ in range(n_new - 1):
        eng.seq_decode(seqs)
    rows = to_np(lg)
    firsts = [_ids(eng, s, 1)[0] for s in seqs]
    for i, p in enumerate(params):
        kw = dict(p or {})
        exp = sampling_ref.sample(rows[i], kw.pop("temperature", 0.0), draw=0, **kw)
        assert firsts[i] == exp, (i, firsts[i], exp)
    assert _ids(eng, seqs[0], n_new) == reqs[0]["ref_ids"]            # the greedy neighbour is its oracle's
    eng.close()


def test_refused_calls_leave_everything_as_it_was(dev):
    from vita_amd._lib import VitaHipError
    n_new = 5
    _, _, eng, (A, B, Cq) = _setup(dev, [70, 70, 70], n_new, seed=8, pool=256, max_seqs=4, max_prefill=256)   # 4 pages, 2 per prompt
    a, b, c, d = (eng.seq_alloc() for _ in range(4))
    eng.seq_free(d)
    total = eng.pages_free()
    assert total == 4

    def refused(seqs, embs, match):
        with pytest.raises(VitaHipError, match=match):
            eng.seq_prefill_batch(seqs, embs)
        assert eng.pages_free() == total and [eng.seq_pos(s) for s in (a, b, c)] == [0, 0, 0]

    refused([a, b, a], [A["emb"][:10], B["emb"][:10], A["emb"][:10]], "twice")
    refused([a, d], [A["emb"], B["emb"]], "not allocated")
    refused([a, b], [torch.cat([A["emb"], A["emb"]]), torch.cat([B["emb"], B["emb"]])], "max_prefill")     # 280 rows > 256
    refused([a, b, c], [A["emb"], B["emb"], Cq["emb"]], "pool exhausted")                                  # dry at the third segment
    eng.seq_prefill_batch([a, b], [A["emb"], B["emb"]])               # the same engine serves a valid call
    assert eng.pages_free() == 0
    for _ in range(n_new - 1):
        eng.seq_decode([a, b])
    assert _ids(eng, a, n_new) == A["ref_ids"] and _ids(eng, b, n_new) == B["ref_ids"]
    eng.close()


def test_int8_experts_in_one_pass(dev):
    """int8 experts: the oracle runs on w' = dequant(quant(w)) (tests/q8_ref.py), as for the single-sequence engine."""
    n_new = 6
    _, _, eng, reqs = _setup(dev, MIXED, n_new, seed=3, experts="int8", oracle_sd=q8_ref.dequant_state_dict)
    assert eng.experts == "int8"
    _one_pass_then_decode(eng, reqs, n_new)
    eng.close()


def test_tensor_parallel_path_with_a_one_rank_collective(dev):
    """force_allreduce = 1 and a 1-rank RCCL communicator: the pass takes the tensor-parallel code (reduce_rows, the overlapped
    column halves on the comm stream) in one process; an all-reduce over one rank is the identity."""
    from vita_amd import _lib
    n_new = 6
    _, _, eng, reqs = _setup(dev, [40, 97, 20, 75], n_new, seed=12, max_seqs=4)
    uid = C.create_string_buffer(128)
    _lib.check(_lib.load().vh_rccl_unique_id(uid), "vh_rccl_unique_id")
    eng.use_rccl(bytes(uid.raw))
    _lib.tune("force_allreduce", 1)
    try:
        _one_pass_then_decode(eng, reqs, n_new)
    finally:
        _lib.tune("force_allreduce", 0)
        eng.close()


@pytest.mark.timeout(900)
def test_released_widths_one_pass_match_the_streamed_oracle(dev):
    """H 4096, 32 / 8 heads, 8 experts of 14336 columns, 2 layers: the mixed list in one call (426 rows: the specialised streaming
    GEMM, the flash kernel's segmented form by the chip-fill rule), then 3 batched decode iterations; every sequence's ids == the
    layer-streamed fp32 oracle's for that sequence alone (oracle/stream.py, teacher-forced over its own tokens)."""
    from oracle import stream
    from vita_amd.checkpoint import synth_mixtral_device
    from vita_amd.engine import MixtralEngine
    n_new, layers, seed = 4, 2, 0
    cfg = VitaConfig()
    cfg.text.num_hidden_layers = layers
    t = cfg.text
    packed = synth_mixtral_device(cfg, dev, seed=seed)
    eng = MixtralEngine(cfg, packed, dev, max_ctx=1024, max_prefill=sum(MIXED), max_new=n_new + 4, max_seqs=6)
    rng = np.random.default_rng(23)
    prompts = [rng.integers(3, t.vocab_size, size=S).tolist() for S in MIXED]
    seqs = [eng.seq_alloc() for _ in prompts]
    eng.seq_prefill_batch(seqs, [packed["embed"][torch.as_tensor(ids, device=dev)].float() for ids in prompts])
    for _ in range(n_new - 1):
        eng.seq_decode(seqs)
    toks = [_ids(eng, q, n_new) for q in seqs]
    eng.close()
    del eng, packed
    torch.cuda.empty_cache()
    fulls = [stream.embed_rows(t, ids + tk[:-1], seed) for ids, tk in zip(prompts, toks)]
    refs = stream.forward_many(t, seed, fulls, n_layers=layers, logits_from=[len(ids) - 1 for ids in prompts])
    for i, (tk, ref) in enumerate(zip(toks, refs)):
        ref_ids = ref["logits"].argmax(-1).tolist()
        assert tk == ref_ids, f"sequence {i} (prompt {MIXED[i]}): device {tk} vs oracle {ref_ids}"


def test_continuous_batcher_groups_prefills_on_the_real_engine(dev):
    from vita_amd.serving import ContinuousBatcher
    n_new = 8
    lens = [40, 97, 64, 130, 20]
    _, _, eng, reqs = _setup(dev, lens, n_new, seed=5, pool=1024, max_seqs=4, max_prefill=256)
    bt = ContinuousBatcher(eng, window=1)
    for i, r in enumerate(reqs):
        bt.add(i, r["emb"], max_tokens=n_new)
    got, fin = {}, {}
    for _ in range(1000):
        if not bt.has_work():
            break
        for rid, new, finished, reason in bt.step():
            got.setdefault(rid, []).extend(new)
            if finished:
                fin[rid] = reason
    assert len(fin) == 5 and bt.stats["failed"] == 0
    for i, r in enumerate(reqs):
        assert got[i] == r["ref_ids"], (i, got[i], r["ref_ids"])
    assert bt.stats["prefills"] == 5 and bt.stats["prefill_calls"] == 3      # (40, 97, 64) | 130 | 20
    assert bt.stats["prefill_calls"] < bt.stats["prefills"] and eng.pages_free() == 1024 // 64
    eng.close()
