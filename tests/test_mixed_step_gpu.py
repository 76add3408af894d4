"""vh_mixtral_seq_step: prompt segments and decode steps in ONE pass over the weights — the decode members' rows ride
behind the prefill segments' rows, gathered from their sequences' state; RoPE + KV write take every row, the segment attention the
prefill rows, the split-KV row kernels (vh_attn_rows) the single rows; the head runs once in prefill mode and once in decode mode.

Bar (tests/test_prefill_batch_gpu.py's, whose geometries and helpers these tests use): every sequence's ids equal the fp32 oracle's
ids for THAT sequence alone, returned score rows within 1e-3, seq_pos / pages_free exact."""
import functools

import numpy as np
import pytest
import torch

from oracle import mixtral as om
from tests import logit_rules_ref as lr
from tests import q4_ref, q8_ref, sampling_ref, seq_scores
from tests.ranks import TP_UNSET, run_ranks
from tests.test_prefill_batch_gpu import FLASH_TEXT
from tests.util import assert_close, to_np
from vita_amd.checkpoint import pack_mixtral, synth_state_dict
from vita_amd.config import TextConfig, VitaConfig

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3
DEQUANT = {"bf16": None, "int8": q8_ref.dequant_state_dict, "mxfp4": q4_ref.dequant_state_dict}
FIRST = (37, 70, 40, 97)        # the first case: two running sequences, two new prompts
FIRST_NEW = 13


@functools.lru_cache(maxsize=None)
def _case(lens, n_new, seed=0, experts="bf16"):
    """weights, prompts and every request's oracle run alone (ids and the raw row of every generated token), computed once per case
    and shared; nothing here is modified afterwards.  n_new: an int, or one count per prompt."""
    cfg = VitaConfig.tiny()
    cfg.text = TextConfig(**FLASH_TEXT)
    sd = synth_state_dict(cfg, seed=seed, parts=("text",))
    orc = om.MixtralOracle(DEQUANT[experts](sd) if DEQUANT[experts] else sd, cfg.text)
    rng = np.random.default_rng(seed + 7)
    counts = [n_new] * len(lens) if isinstance(n_new, int) else list(n_new)
    reqs = []
    for S, n in zip(lens, counts):
        emb = sd["model.embed_tokens.weight"][rng.integers(3, cfg.text.vocab_size, size=S)]
        orc.reset()
        ids, rows = orc.greedy(emb, n)
        reqs.append(dict(emb=emb, ref_ids=ids, ref_lg=np.stack(rows)))
    return cfg, sd, reqs


def _engine(dev, cfg, sd, experts="bf16", pool=2048, max_prefill=256, max_new=32, max_seqs=6, **kw):
    from vita_amd.engine import MixtralEngine
    packed = pack_mixtral(sd, cfg, dev, experts=experts) if experts != "bf16" else pack_mixtral(sd, cfg, dev)
    return MixtralEngine(cfg, packed, dev, max_ctx=pool, max_prefill=max_prefill, max_new=max_new, max_seqs=max_seqs, **kw)


@pytest.fixture
def flash():
    """attn_fa forced, as the `flash` cases of tests/test_prefill_batch_gpu.py: the prefill segments of every pass take k_attn_fa"""
    from vita_amd import _lib
    _lib.tune("attn_fa", 2)
    yield
    _lib.tune("attn_fa", 1)


def _emb(r, dev):
    return torch.from_numpy(r["emb"]).to(dev)


def _ids(eng, s, n):
    torch.cuda.synchronize()
    eng.check_device_flag(eng.seq_counters(s).tolist())
    return eng.seq_tokens(s)[:n].tolist()


def _first_script(eng, reqs, dev, gather=True):
    """A (37) and B (70) run for three iterations; ONE seq_step prefills C (40) and D (97) and advances A and B; then plain
    iterations of all four until C and D have 10 tokens.  -> (slots, the call's score rows, state right after the call)."""
    A, B, Cq, Dq = reqs
    a, b = eng.seq_alloc(), eng.seq_alloc()
    eng.seq_prefill_batch([a, b], [_emb(A, dev), _emb(B, dev)])
    for _ in range(2):
        eng.seq_decode([a, b])
    c, d = eng.seq_alloc(), eng.seq_alloc()
    free0 = eng.pages_free()
    lg = eng.seq_step([c, d], [_emb(Cq, dev), _emb(Dq, dev)], [a, b], want_logits=gather)
    torch.cuda.synchronize()
    after = dict(pos=[eng.seq_pos(s) for s in (a, b, c, d)], ngen=[int(eng.seq_counters(s)[1]) for s in (a, b, c, d)],
                 dpos=[int(eng.seq_counters(s)[0]) for s in (a, b, c, d)], tok3=[int(eng.seq_tokens(s)[3]) for s in (a, b)],
                 pages=free0 - eng.pages_free())
    for _ in range(9):
        eng.seq_decode([a, b, c, d])
    return (a, b, c, d), lg, after


def _check_first(eng, reqs, slots, lg, after):
    A, B, Cq, Dq = reqs
    a, b, c, d = slots
    # positions: prompt + tokens fed back; counters: the decode members went ON (4 tokens, the fourth appended), the new ones restarted
    assert after["pos"] == [37 + 3, 70 + 3, 40, 97] and after["dpos"] == after["pos"], after
    assert after["ngen"] == [4, 4, 1, 1], after
    assert after["tok3"] == [A["ref_ids"][3], B["ref_ids"][3]], after
    assert after["pages"] == 1 + 2                      # C: one page, D: two; A (40 keys) and B (73 keys) stay inside theirs
    if lg is not None:
        assert tuple(lg.shape) == (4, eng.c.vocab)
        rows = to_np(lg)
        assert_close("first token of C", rows[0], Cq["ref_lg"][0], atol=LOGIT_TOL)
        assert_close("first token of D", rows[1], Dq["ref_lg"][0], atol=LOGIT_TOL)
        assert_close("decode row of A", rows[2], A["ref_lg"][3], atol=LOGIT_TOL)
        assert_close("decode row of B", rows[3], B["ref_lg"][3], atol=LOGIT_TOL)
    for name, s, r, n in (("A", a, A, 13), ("B", b, B, 13), ("C", c, Cq, 10), ("D", d, Dq, 10)):
        assert _ids(eng, s, n) == r["ref_ids"][:n], f"sequence {name} differs from its oracle"
        assert eng.seq_pos(s) == r["emb"].shape[0] + n - 1


def test_mixed_pass_matches_the_oracles(dev, flash):
    cfg, sd, reqs = _case(FIRST, FIRST_NEW)
    eng = _engine(dev, cfg, sd)
    total = eng.pages_free()
    slots, lg, after = _first_script(eng, reqs, dev)
    _check_first(eng, reqs, slots, lg, after)
    for s in slots:
        eng.seq_free(s)
    assert eng.pages_free() == total
    eng.close()


def test_single_rows_through_the_segment_attention(dev, flash):
    """vh_tune("step_attn", 0): the decode rows as 1-row segments of the segment attention — the same bar."""
    from vita_amd import _lib
    cfg, sd, reqs = _case(FIRST, FIRST_NEW)
    eng = _engine(dev, cfg, sd)
    _lib.tune("step_attn", 0)
    try:
        slots, lg, after = _first_script(eng, reqs, dev)
        _check_first(eng, reqs, slots, lg, after)
    finally:
        _lib.tune("step_attn", 1)
        eng.close()


def test_decode_members_cross_page_boundaries_inside_mixed_calls(dev, flash):
    """prompts of 63, 64 and 65 rows stepped ONLY by seq_step across positions 64 and 128: decode-only calls alternate with calls
    that also prefill a fresh 20-row prompt (a new sequence each time).  New pages are taken inside mixed calls."""
    n_new = 68
    cfg, sd, reqs = _case((63, 64, 65, 20), (n_new, n_new, n_new, 1), seed=3)
    members, F = reqs[:3], reqs[3]
    eng = _engine(dev, cfg, sd, max_prefill=256, max_new=n_new + 4)
    seqs = [eng.seq_alloc() for _ in members]
    eng.seq_prefill_batch(seqs, [_emb(r, dev) for r in members])
    grown = {False: 0, True: 0}            # pages the members took, by "the call had a prompt segment"
    f_emb = _emb(F, dev)
    for it in range(n_new - 1):
        mixed = it % 2 == 1
        before = [len(eng.seq_pages(s)) for s in seqs]
        if mixed:
            f = eng.seq_alloc()
            eng.seq_step([f], [f_emb], seqs)
            assert _ids(eng, f, 1) == F["ref_ids"] and eng.seq_pos(f) == 20
            eng.seq_free(f)
        else:
            eng.seq_step([], [], seqs)
        grown[mixed] += sum(len(eng.seq_pages(s)) - n0 for s, n0 in zip(seqs, before))
    for s, r in zip(seqs, members):
        S = r["emb"].shape[0]
        assert _ids(eng, s, n_new) == r["ref_ids"], f"the {S}-row prompt differs from its oracle"
        assert eng.seq_pos(s) == S + n_new - 1 and eng.seq_pos(s) > 128 and len(eng.seq_pages(s)) == 3
    assert grown[True] >= 1 and grown[False] >= 1 and grown[True] + grown[False] == 5, grown
    eng.close()


def test_a_prompt_in_three_chunks_next_to_two_decoding_sequences(dev, flash):
    """150 rows as 60 + 60 + 30 over three consecutive seq_step calls in which two other sequences decode; the chunked sequence's
    first token comes from the third call."""
    n_new = 9
    cfg, sd, (P, A, B) = _case((150, 37, 70), n_new, seed=4)
    eng = _engine(dev, cfg, sd)
    a, b = eng.seq_alloc(), eng.seq_alloc()
    eng.seq_prefill_batch([a, b], [_emb(A, dev), _emb(B, dev)])
    eng.seq_decode([a, b])
    p = eng.seq_alloc()
    pe = _emb(P, dev)
    for lo, hi in ((0, 60), (60, 120), (120, 150)):
        lg = eng.seq_step([p], [pe[lo:hi]], [a, b], want_logits=True)
        assert eng.seq_pos(p) == hi
    assert_close("first token of the chunked prompt", to_np(lg[0]), P["ref_lg"][0], atol=LOGIT_TOL)
    assert_close("A's decode row in the third call", to_np(lg[1]), A["ref_lg"][4], atol=LOGIT_TOL)
    torch.cuda.synchronize()
    assert int(eng.seq_counters(p)[1]) == 1 and _ids(eng, p, 1) == P["ref_ids"][:1]
    assert int(eng.seq_counters(a)[1]) == 5
    for _ in range(n_new - 5):
        eng.seq_decode([a, b, p])
    assert _ids(eng, a, n_new) == A["ref_ids"] and _ids(eng, b, n_new) == B["ref_ids"]
    assert _ids(eng, p, n_new - 4) == P["ref_ids"][:n_new - 4]
    eng.close()


def test_decode_only_pass_of_five(dev, flash):
    """n_pf == 0 with five members (more than the VH_BMAX = 4 lanes of the batched decode kernels): every step a seq_step."""
    n_new = 8
    lens = (5, 40, 63, 64, 97)
    cfg, sd, reqs = _case(lens, n_new, seed=5)
    eng = _engine(dev, cfg, sd, max_prefill=320)
    seqs = [eng.seq_alloc() for _ in reqs]
    eng.seq_prefill_batch(seqs, [_emb(r, dev) for r in reqs])
    for it in range(1, n_new):
        lg = eng.seq_step([], [], seqs, want_logits=True)
        for i, r in enumerate(reqs):
            assert_close(f"step {it} of the {lens[i]}-row prompt", to_np(lg[i]), r["ref_lg"][it], atol=LOGIT_TOL)
    for s, r in zip(seqs, reqs):
        assert _ids(eng, s, n_new) == r["ref_ids"] and eng.seq_pos(s) == r["emb"].shape[0] + n_new - 1
    eng.close()


def test_prefill_only_call_is_seq_prefill_batch(dev):
    outs = []
    cfg, sd, reqs = _case((40, 97, 64), 3, seed=6)
    for step in (False, True):
        eng = _engine(dev, cfg, sd)
        seqs = [eng.seq_alloc() for _ in reqs]
        embs = [_emb(r, dev) for r in reqs]
        lg = eng.seq_step(seqs, embs, [], want_logits=True) if step else eng.seq_prefill_batch(seqs, embs, want_logits=True)
        eng.seq_decode(seqs)
        outs.append(([_ids(eng, s, 2) for s in seqs], lg.clone(), [eng.seq_pos(s) for s in seqs], [eng.seq_pages(s) for s in seqs],
                     eng.pages_free()))
        assert outs[-1][0] == [r["ref_ids"][:2] for r in reqs]
        eng.close()
    assert outs[0][0] == outs[1][0] and outs[0][2:] == outs[1][2:] and torch.equal(outs[0][1], outs[1][1])


def _forced_rows(cfg, sd, emb, tokens):
    """the oracle's raw rows of every generated token, teacher-forced over the device's own tokens"""
    orc = om.MixtralOracle(sd, cfg.text)
    x = np.concatenate([emb, sd["model.embed_tokens.weight"][np.asarray(tokens[:-1], np.int64)]]) if len(tokens) > 1 else emb
    logits, _ = orc.forward(x)
    return logits[emb.shape[0] - 1:]


def test_sampling_and_logit_rules_continue_across_a_mixed_call(dev, flash):
    """A draws with seeded temperature / top-k / top-p, B carries repetition + frequency penalties and logprobs = 5, C is greedy; all
    three are decode members of a mixed call that prefills D.  The draw index, the penalty table and the logprob rows go on: the
    mixed call's tokens are the contract's picks (tests/sampling_ref.py, tests/logit_rules_ref.py) from the call's own returned rows
    at draw index 3 / under the table of the first three tokens, and every token of the run is the pick from the oracle's row
    (teacher-forced over the device's tokens) unless the oracle's row has the two best candidates within what a 1e-3 logit error
    can swap."""
    n_new, K = 8, 5
    cfg, sd, (A, B, Cq, Dq) = _case(FIRST, FIRST_NEW)
    V = cfg.text.vocab_size
    eng = _engine(dev, cfg, sd, penalty_tables=True, max_logprobs=K)
    samp = dict(temperature=0.8, top_k=20, top_p=0.9, seed=5)
    pen = dict(r=1.3, f=0.6)
    a, b, c = (eng.seq_alloc() for _ in range(3))
    eng.seq_set_sampling(a, **samp)
    eng.seq_set_logit_rules(b, repetition_penalty=pen["r"], frequency_penalty=pen["f"], logprobs=K)
    eng.seq_prefill_batch([a, b, c], [_emb(A, dev), _emb(B, dev), _emb(Cq, dev)])
    for _ in range(2):
        eng.seq_decode([a, b, c])
    d = eng.seq_alloc()
    lg = to_np(eng.seq_step([d], [_emb(Dq, dev)], [a, b, c], want_logits=True))
    for _ in range(n_new - 4):
        eng.seq_decode([a, b, c, d])
    ta, tb = _ids(eng, a, n_new), _ids(eng, b, n_new)
    assert _ids(eng, c, n_new) == Cq["ref_ids"][:n_new] and _ids(eng, d, n_new - 3) == Dq["ref_ids"][:n_new - 3]
    assert int(eng.seq_counters(a)[1]) == n_new and int(eng.seq_counters(b)[1]) == n_new
    # the mixed call itself, on its own rows: draw index 3, the table of tokens 0 .. 2
    assert ta[3] == sampling_ref.sample(lg[1], samp["temperature"], samp["top_k"], samp["top_p"], samp["seed"], 3)
    assert tb[3] == int(np.argmax(lr.penalise(lg[2], lr.seen_table(V, (), tb[:3]), **pen)))
    # the whole run against the oracle's rows
    ra, rb = _forced_rows(cfg, sd, A["emb"], ta), _forced_rows(cfg, sd, B["emb"], tb)
    assert_close("A's row of the mixed call", lg[1], ra[3], atol=LOGIT_TOL)
    assert_close("B's row of the mixed call", lg[2], rb[3], atol=LOGIT_TOL)
    for i in range(n_new):
        args = (ra[i], samp["temperature"], samp["top_k"], samp["top_p"], samp["seed"], i)
        assert ta[i] == sampling_ref.sample(*args) or sampling_ref.top2_gap(*args) < 2 * LOGIT_TOL / samp["temperature"], (i, ta)
        x = np.sort(lr.penalise(rb[i], lr.seen_table(V, (), tb[:i]), **pen).astype(np.float64))
        assert tb[i] == int(np.argmax(lr.penalise(rb[i], lr.seen_table(V, (), tb[:i]), **pen))) or x[-1] - x[-2] < 2 * LOGIT_TOL * pen["r"], (i, tb)
    lp = tuple(t.cpu().numpy().copy() for t in eng.logprobs(b))
    worst = seq_scores.check_sequence(rb, tb, lp, K, LOGIT_TOL, what="B")
    print(f"worst log-probability error {worst:.2e} (bound {2 * LOGIT_TOL:.0e})")
    seen = eng.seen_table(b).cpu().numpy().astype(np.uint32)
    assert np.array_equal(seen & np.uint32(0x7FFFFFFF), lr.seen_table(V, (), tb))
    eng.close()


@pytest.mark.parametrize("experts", ["int8", "mxfp4"])
def test_quantised_experts_in_a_mixed_pass(dev, flash, experts):
    """the first case on int8 / MXFP4 experts: the oracle runs on the dequantised weights the engine computes with."""
    cfg, sd, reqs = _case(FIRST, FIRST_NEW, 0, experts)
    eng = _engine(dev, cfg, sd, experts=experts)
    assert eng.experts == experts
    slots, lg, after = _first_script(eng, reqs, dev)
    _check_first(eng, reqs, slots, lg, after)
    eng.close()


def test_refused_calls_leave_everything_as_it_was(dev):
    from vita_amd._lib import VitaHipError
    n_new = 4
    cfg, sd, (A, B, Cq) = _case((70, 70, 70), n_new, seed=8)
    eng = _engine(dev, cfg, sd, pool=320, max_prefill=128, max_seqs=5)       # 5 pages, 2 per prompt
    a, b, c, d, e = (eng.seq_alloc() for _ in range(5))
    eng.seq_free(e)
    eng.seq_prefill(a, _emb(A, dev))
    eng.seq_prefill(b, _emb(B, dev))
    eng.seq_decode([a, b])
    total = eng.pages_free()
    assert total == 1
    state = lambda: ([eng.seq_pos(s) for s in (a, b, c, d)], eng.pages_free(), [_ids(eng, s, 2) for s in (a, b)])
    s0 = state()
    ce = _emb(Cq, dev)

    def refused(pf, embs, dec, match):
        with pytest.raises(VitaHipError, match=match):
            eng.seq_step(pf, embs, dec)
        assert state() == s0

    refused([c], [ce[:10]], [a, c], "twice")                         # a slot in both lists
    refused([c], [ce[:10]], [a, a], "twice")                         # a decode member twice
    refused([c, c], [ce[:10], ce[:10]], [a], "twice")
    refused([c], [torch.cat([ce, ce])[:127]], [a, b], "max_prefill")  # 127 + 2 rows > 128
    refused([c], [ce[:10]], [a, d], "no prompt")                     # a decode member without a prompt
    refused([c], [ce[:10]], [e], "not allocated")
    refused([c], [ce], [a, b], "pool exhausted")                     # C needs two pages, one is free
    with pytest.raises(ValueError):
        eng.seq_step([], [], [])
    with pytest.raises(ValueError):
        eng.seq_step([c], [], [a])
    lib = eng.lib
    import ctypes as C
    one = (C.c_int * 1)(c)
    assert lib.vh_mixtral_seq_step(eng.h, one, one, 1, None, None, 0, None, None) == -2       # null embeds with a prompt segment
    assert lib.vh_mixtral_seq_step(eng.h, None, None, 0, None, None, 1, None, None) == -2     # null decode list
    assert lib.vh_mixtral_seq_step(eng.h, None, None, 0, None, None, 0, None, None) == -2     # no member at all
    assert state() == s0
    eng.seq_step([c], [ce[:60]], [a, b])                              # the same engine serves a valid call (one page)
    assert eng.pages_free() == 0 and eng.seq_pos(c) == 60
    assert _ids(eng, a, 3) == A["ref_ids"][:3] and _ids(eng, b, 3) == B["ref_ids"][:3]
    eng.close()


def test_a_failed_pass_poisons_exactly_the_listed_slots(dev):
    """a pass that fails after its first enqueue (the tensor-parallel path with no collective installed: the first all-reduce is
    refused on the host) loses exactly the listed sequences: they are refused from then on, their neighbours go on."""
    from vita_amd import _lib
    from vita_amd._lib import VitaHipError
    n_new = 5
    cfg, sd, (A, B, Cq, X) = _case((37, 70, 40, 20), n_new, seed=9)
    eng = _engine(dev, cfg, sd)
    a, b, c = (eng.seq_alloc() for _ in range(3))
    eng.seq_prefill_batch([a, b, c], [_emb(r, dev) for r in (A, B, Cq)])
    x = eng.seq_alloc()
    _lib.tune("force_allreduce", 1)
    try:
        with pytest.raises(VitaHipError, match="all-reduce"):
            eng.seq_step([x], [_emb(X, dev)], [a])
    finally:
        _lib.tune("force_allreduce", 0)
    torch.cuda.synchronize()
    pos = [eng.seq_pos(s) for s in (a, b, c, x)]
    for pf, embs, dec in (([], [], [a, b]), ([x], [_emb(X, dev)], [b]), ([], [], [a])):
        with pytest.raises(VitaHipError, match="previous step failed"):
            eng.seq_step(pf, embs, dec)
        assert [eng.seq_pos(s) for s in (a, b, c, x)] == pos
    for _ in range(n_new - 1):
        eng.seq_step([], [], [b, c])
    assert _ids(eng, b, n_new) == B["ref_ids"] and _ids(eng, c, n_new) == Cq["ref_ids"]
    eng.seq_free(a)
    eng.seq_free(x)
    y = eng.seq_alloc()                                 # a freed slot is clean again
    eng.seq_step([y], [_emb(X, dev)], [])
    assert _ids(eng, y, 1) == X["ref_ids"][:1]
    eng.close()


@pytest.mark.timeout(900)
def test_released_widths_mixed_pass_matches_the_streamed_oracle(dev):
    """H 4096, 32 / 8 heads, 8 experts of 14336 columns, 2 layers: three running sequences plus prompts of 64 and 130 rows in one
    mixed pass (the real GEMM tiles, the row kernels at G = 4 with 8 KV heads), then two plain iterations; every sequence's ids ==
    the layer-streamed fp32 oracle's for that sequence alone (oracle/stream.py, teacher-forced over its own tokens)."""
    from oracle import stream
    from vita_amd.checkpoint import synth_mixtral_device
    from vita_amd.engine import MixtralEngine
    layers, seed = 2, 0
    lens, new = [20, 33, 70, 64, 130], [64, 130]
    cfg = VitaConfig()
    cfg.text.num_hidden_layers = layers
    t = cfg.text
    packed = synth_mixtral_device(cfg, dev, seed=seed)
    eng = MixtralEngine(cfg, packed, dev, max_ctx=1024, max_prefill=256, max_new=8, max_seqs=6)
    rng = np.random.default_rng(29)
    prompts = [rng.integers(3, t.vocab_size, size=S).tolist() for S in lens]
    emb = lambda ids: packed["embed"][torch.as_tensor(ids, device=dev)].float()
    run = [eng.seq_alloc() for _ in range(3)]
    eng.seq_prefill_batch(run, [emb(p) for p in prompts[:3]])
    eng.seq_decode(run)
    fresh = [eng.seq_alloc() for _ in new]
    eng.seq_step(fresh, [emb(p) for p in prompts[3:]], run)
    for _ in range(2):
        eng.seq_decode(run + fresh)
    toks = [_ids(eng, q, 5) for q in run] + [_ids(eng, q, 3) for q in fresh]
    assert [eng.seq_pos(q) for q in run + fresh] == [S + len(tk) - 1 for S, tk in zip(lens, toks)]
    eng.close()
    del eng, packed
    torch.cuda.empty_cache()
    fulls = [stream.embed_rows(t, ids + tk[:-1], seed) for ids, tk in zip(prompts, toks)]
    refs = stream.forward_many(t, seed, fulls, n_layers=layers, logits_from=[len(ids) - 1 for ids in prompts])
    for i, (tk, ref) in enumerate(zip(toks, refs)):
        ref_ids = ref["logits"].argmax(-1).tolist()
        assert tk == ref_ids, f"sequence {i} (prompt {lens[i]}): device {tk} vs oracle {ref_ids}"


def _tp_worker(ctx):
    from vita_amd import _lib
    from vita_amd.engine import MixtralEngine
    from vita_amd.parallel import setup_tensor_parallel
    rank, world, dev = ctx.rank, ctx.world, ctx.dev
    cfg, sd, reqs = _case(FIRST, FIRST_NEW)
    packed = pack_mixtral(sd, cfg, dev, rank=rank, world=world)
    eng = MixtralEngine(cfg, packed, dev, max_ctx=2048, max_prefill=256, max_new=32, rank=rank, world=world, max_seqs=6)
    ctx.defer(eng.close)
    name = setup_tensor_parallel(eng, rank, world, dev, backend="gloo")
    _lib.tune("attn_fa", 2)
    slots, lg, after = _first_script(eng, reqs, dev)
    ids = [_ids(eng, s, n) for s, n in zip(slots, (13, 13, 10, 10))]
    return name, ids, after, lg.cpu().numpy()


def test_tensor_parallel_world_2_mixed_pass(dev):
    """two engine processes on one GPU run the first case: ids equal on both ranks and equal to the unsharded oracle's, the call's
    gathered score rows within 1e-3."""
    r0, r1 = run_ranks(_tp_worker, 2, env=TP_UNSET, deadline_s=120)
    cfg, sd, reqs = _case(FIRST, FIRST_NEW)
    assert r0[0] == r1[0], (r0[0], r1[0])
    assert r0[1] == r1[1] == [r["ref_ids"][:n] for r, n in zip(reqs, (13, 13, 10, 10))]
    assert r0[2] == r1[2] and r0[2]["ngen"] == [4, 4, 1, 1] and r0[2]["pos"] == [40, 73, 40, 97]
    assert np.array_equal(r0[3], r1[3])
    for i, (r, step) in enumerate(((reqs[2], 0), (reqs[3], 0), (reqs[0], 3), (reqs[1], 3))):
        assert_close(f"row {i} of the mixed call under TP 2", r0[3][i], r["ref_lg"][step], atol=LOGIT_TOL)
