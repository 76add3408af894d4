"""Penalties and log-probabilities on the device (vh_logit_rules) against their numpy restatement
(tests/logit_rules_ref.py): the per-operator entry on caller-provided rows, the engine's generate() across lookahead windows (greedy,
temperature-only and filtered sampling), multi-step decode, "off is off", three sequences in one batched iteration, recompute
preemption, and what the setters refuse."""
import asyncio

import numpy as np
import pytest
import torch

from tests import logit_rules_ref as ref
from tests import sampling_ref
from vita_amd import ops
from vita_amd.checkpoint import synth_state_dict
from vita_amd.config import VitaConfig

pytestmark = pytest.mark.gpu

PROMPT_BIT = np.uint32(0x80000000)


def _ulp_ok(got, exp):
    """every entry within 1 fp32 ulp (np.spacing) of the restatement; infinities and NaN equal as such.  -> (ok, worst in ulps)"""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    fin = np.isfinite(exp)
    same = np.array_equal(got[~fin], exp[~fin], equal_nan=True)
    if not fin.any():
        return same, 0.0
    d = np.abs(got[fin].astype(np.float64) - exp[fin].astype(np.float64)) / np.spacing(np.abs(exp[fin])).astype(np.float64)
    return bool(same and np.isfinite(got[fin]).all() and d.max() <= 1.0), float(d.max())


# ---- 1. the operator against the restatement ------------------------------------------------------------------------------
def _case_rows(V, rng):
    rows = np.stack([(rng.standard_normal(V) * 2.5).astype(np.float32) for _ in range(6)])
    rows[1, rng.integers(0, V, min(V, 40))] = rows[1].max()            # tied maxima
    rows[2] = np.round(rows[2] * 4) / 4                                # values on a 1/4 grid: ties everywhere, zeros of both signs
    rows[3] = np.nan
    rows[4] = -np.inf
    rows[5] = np.nan
    rows[5, [0, V - 1]] = [1.0, 2.0]                                   # two finite entries among NaN (one when V = 1)
    return rows


def _histories(V, rng):
    sub = rng.permutation(V)[:max(1, V // 3)]
    counts = np.zeros(V, np.uint32)
    ids = rng.permutation(V)[:min(V, 600)]
    counts[ids] = (np.arange(len(ids)) % 300 + 1).astype(np.uint32)    # counts 1 .. 300
    both = counts.copy()
    both[ids[::2]] |= PROMPT_BIT                                       # ids that are in the prompt AND in the output
    prompt_only = np.zeros(V, np.uint32)
    prompt_only[sub] = PROMPT_BIT
    return {"empty": np.zeros(V, np.uint32), "all prompt": np.full(V, PROMPT_BIT, np.uint32), "prompt only": prompt_only,
            "counts": counts, "both": both}


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 1023, 1025, 51760])
def test_operator_equals_the_restatement(V):
    rng = np.random.default_rng(1000 + V)
    rows = _case_rows(V, rng)
    t = torch.from_numpy(rows).cuda()
    bad = []
    for name, seen in _histories(V, rng).items():
        ts = torch.from_numpy(seen.view(np.int32)).cuda()
        for r in (0.5, 1.0, 1.3):
            for f in (-0.5, 0.0, 0.7):
                for p in (0.0, 1.1):
                    got = ops.logit_rules_rows(t, ts, r, p, f)[0].cpu().numpy()
                    exp = np.stack([ref.penalise(row, seen, r=r, f=f, p=p) for row in rows])
                    if not np.array_equal(got.view(np.uint32), exp.view(np.uint32)):
                        bad.append((name, r, f, p, int((got.view(np.uint32) != exp.view(np.uint32)).sum())))
    assert not bad, f"penalised rows differ from the restatement (history, r, f, p, entries): {bad[:8]}"
    raw = ops.logit_rules_rows(t, None, 1.3, 1.1, 0.7)[0].cpu().numpy()            # no table: the rows come back untouched
    assert np.array_equal(raw.view(np.uint32), rows.view(np.uint32))
    toks = np.array([int(rng.integers(0, V)) for _ in range(6)], np.int32)
    toks[0] = int(np.argmax(rows[0]))
    worst = 0.0
    for K in (0, 1, 5, 20):                                                        # K > V included
        _, lp, ids, top = ops.logit_rules_rows(t, None, tokens=torch.from_numpy(toks).cuda(), logprobs=K, want_penalised=False)
        lp, ids, top = lp.cpu().numpy(), ids.cpu().numpy(), top.cpu().numpy()
        for i, row in enumerate(rows):
            e_lp, e_ids, e_top = ref.logprobs(row, toks[i], K)
            assert ids[i].tolist() == e_ids.tolist(), (V, K, i, ids[i], e_ids)
            ok1, w1 = _ulp_ok(lp[i:i + 1], [e_lp])
            ok2, w2 = _ulp_ok(top[i], e_top)
            worst = max(worst, w1, w2)
            assert ok1 and ok2, (V, K, i, w1, w2, lp[i], e_lp, top[i], e_top)
    print(f"V {V}: logprobs within {worst:.2f} ulp of the restatement")


def test_operator_on_rows_past_the_register_path():
    """rows of more than 1024 x 52 entries take the logprob kernel's other path (the winner's owner re-reads the row); same contract"""
    V = 53251
    rng = np.random.default_rng(V)
    rows = _case_rows(V, rng)[:3]
    t = torch.from_numpy(rows).cuda()
    seen = _histories(V, rng)["both"]
    got = ops.logit_rules_rows(t, torch.from_numpy(seen.view(np.int32)).cuda(), 1.3, 1.1, 0.7)[0].cpu().numpy()
    exp = np.stack([ref.penalise(row, seen, r=1.3, f=0.7, p=1.1) for row in rows])
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    toks = np.array([int(np.argmax(rows[0])), 7, V - 1], np.int32)
    _, lp, ids, top = ops.logit_rules_rows(t, None, tokens=torch.from_numpy(toks).cuda(), logprobs=20, want_penalised=False)
    for i, row in enumerate(rows):
        e_lp, e_ids, e_top = ref.logprobs(row, toks[i], 20)
        assert ids[i].tolist() == e_ids.tolist()
        assert _ulp_ok(lp[i:i + 1].cpu().numpy(), [e_lp])[0] and _ulp_ok(top[i].cpu().numpy(), e_top)[0]


# ---- 2-4. the engine ------------------------------------------------------------------------------------------------------
SEED, PROMPT_SEED = 41, 6     # a synthetic model whose greedy run repeats tokens within 20 steps (checked on the numpy oracle: 8 distinct
                              # ids of 20, top-2 gaps >= 0.026 in the greedy and in both penalised runs), so that the penalties change the ids


def _prompt():
    return np.random.default_rng(PROMPT_SEED).integers(3, VitaConfig.tiny().text.vocab_size, size=37)


@pytest.fixture(scope="module")
def tiny(dev):
    from vita_amd.model import build_synthetic_model
    model, sd = build_synthetic_model(VitaConfig.tiny(), seed=SEED, device=dev, max_new_tokens=32, max_prefill=512,
                                      penalty_tables=True, max_logprobs=5)
    emb = torch.from_numpy(sd["model.embed_tokens.weight"][_prompt()]).to(dev)[None].float()
    return model, emb


@pytest.fixture(scope="module")
def tiny_plain(dev):
    """the same model on an engine created WITHOUT tables and logprob buffers"""
    from vita_amd.model import build_synthetic_model
    model, _ = build_synthetic_model(VitaConfig.tiny(), seed=SEED, device=dev, max_new_tokens=32, max_prefill=512)
    return model


def _gen(model, emb, n=20, **kw):
    out = model.generate(inputs_embeds=emb, max_new_tokens=n, eos_token_id=-1, return_dict_in_generate=True, output_scores=True, **kw)
    torch.cuda.synchronize()
    return out.sequences[0].tolist(), [s[0].cpu().numpy() for s in out.scores], getattr(out, "logprobs", None)


def _penalised(scores, ids, prompt=(), **pen):
    V = scores[0].shape[0]
    return [ref.penalise(scores[i], ref.seen_table(V, prompt, ids[:i]), **pen) for i in range(len(ids))]


def _check_logprobs(lps, scores, ids, K):
    assert len(lps) == len(ids)
    worst = 0.0
    for i, d in enumerate(lps):
        e_lp, e_ids, e_top = ref.logprobs(scores[i], ids[i], K)
        exp = {int(v): float(x) for v, x in zip(e_ids, e_top) if v >= 0}
        exp.setdefault(int(ids[i]), float(e_lp))
        assert list(d)[:K] == [int(v) for v in e_ids if v >= 0], (i, list(d), e_ids)      # the top K, in order
        assert set(d) == set(exp), (i, d, exp)
        ok, w = _ulp_ok([d[k] for k in exp], [exp[k] for k in exp])
        worst = max(worst, w)
        assert ok, (i, w, d, exp)
    return worst


def test_generate_with_repetition_penalty_and_logprobs(tiny):
    model, emb = tiny
    greedy0, _, none = _gen(model, emb)
    assert none is None
    ids, scores, lps = _gen(model, emb, repetition_penalty=1.3, output_logprobs=5)
    assert len(ids) == 20 and len(scores) == 20                                   # crosses two lookahead windows of 8
    exp = [int(np.argmax(x)) for x in _penalised(scores, ids, r=1.3)]             # HF semantics on inputs_embeds: generated ids only
    assert ids == exp, (ids, exp)
    assert ids != greedy0
    print("logprobs worst ulp", _check_logprobs(lps, scores, ids, 5))
    assert _gen(model, emb)[0] == greedy0                                         # off again afterwards
    with pytest.raises(ValueError):
        model.generate(inputs_embeds=emb, max_new_tokens=4, output_logprobs=6)    # above the model's max_logprobs


def test_generate_with_frequency_presence_and_a_prompt_set(tiny):
    model, emb = tiny
    prompt = _prompt().tolist()
    greedy0 = _gen(model, emb)[0]
    kw = dict(repetition_penalty=1.3, frequency_penalty=0.6, presence_penalty=0.4, penalty_prompt_ids=prompt)
    ids, scores, lps = _gen(model, emb, output_logprobs=5, **kw)
    exp = [int(np.argmax(x)) for x in _penalised(scores, ids, prompt, r=1.3, f=0.6, p=0.4)]
    assert ids == exp and ids != greedy0, (ids, exp, greedy0)
    _check_logprobs(lps, scores, ids, 5)
    ids2, scores2, _ = _gen(model, emb, frequency_penalty=0.6, presence_penalty=0.4)       # r = 1: steps 2 and 3 alone, no prompt set
    assert ids2 == [int(np.argmax(x)) for x in _penalised(scores2, ids2, r=1.0, f=0.6, p=0.4)] and ids2 != greedy0


@pytest.mark.parametrize("params", [dict(temperature=1.3, top_k=0, top_p=1.0), dict(temperature=0.8, top_k=12, top_p=0.9)])
def test_generate_samples_from_the_penalised_rows(tiny, params):
    """seeded temperature-only sampling (the Gumbel compare inside the LM head) and top-k + top-p (the filter kernel) see the
    penalised values; the kept scores stay raw."""
    model, emb = tiny
    prompt = _prompt().tolist()
    ids, scores, lps = _gen(model, emb, do_sample=True, seed=1234, repetition_penalty=1.3, frequency_penalty=0.6, presence_penalty=0.4,
                            penalty_prompt_ids=prompt, output_logprobs=3, **params)
    rows = _penalised(scores, ids, prompt, r=1.3, f=0.6, p=0.4)
    exp = [sampling_ref.sample(rows[i], params["temperature"], params["top_k"], params["top_p"], 1234, i) for i in range(20)]
    assert ids == exp, (ids, exp)
    _check_logprobs(lps, scores, ids, 3)
    # at this model's small logits the vLLM-range penalties rarely move a draw; a strongly NEGATIVE presence / frequency penalty (the
    # C layer takes any finite value) pulls the draws onto tokens already generated, so a path that ignored the table would show
    plain = _gen(model, emb, do_sample=True, seed=1234, **params)
    assert plain[0] == [sampling_ref.sample(plain[1][i], params["temperature"], params["top_k"], params["top_p"], 1234, i) for i in range(20)]
    ids, scores, lps = _gen(model, emb, do_sample=True, seed=1234, presence_penalty=-6.0, frequency_penalty=-1.0, output_logprobs=3, **params)
    rows = _penalised(scores, ids, r=1.0, f=-1.0, p=-6.0)
    exp = [sampling_ref.sample(rows[i], params["temperature"], params["top_k"], params["top_p"], 1234, i) for i in range(20)]
    assert ids == exp, (ids, exp)
    assert ids != plain[0] and len(set(ids)) < len(set(plain[0]))
    _check_logprobs(lps, scores, ids, 3)


def test_multi_step_decode_equals_single_steps(tiny):
    model, emb = tiny
    eng = model.engine
    prompt = _prompt().tolist()
    runs = []
    for steps in ([8], [1] * 8):
        eng.reset()
        eng.set_sampling()
        eng.set_logit_rules(1.3, 0.4, 0.6, 5, prompt_ids=prompt)
        eng.prefill(emb[0])
        for n in steps:
            eng.decode(n)
        torch.cuda.synchronize()
        tok, top_id, top = eng.logprobs()
        runs.append((eng.generated(), tok[:9].cpu().numpy().copy(), top_id[:9].cpu().numpy().copy(), top[:9].cpu().numpy().copy(),
                     eng.seen_table().cpu().numpy().copy()))
    eng.reset()
    a, b = runs
    assert len(a[0]) == 9 and a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(a[4].view(np.uint32), ref.seen_table(a[4].shape[0], prompt, a[0]))     # the table is the history
    assert np.isfinite(a[1]).all() and (a[1] < 0).all()


def test_off_is_off(tiny, tiny_plain):
    """an engine created with tables and max_logprobs = 5 under neutral rules against one created without: ids and kept logits
    rows bit-identical over 20 steps."""
    model, emb = tiny
    a = _gen(model, emb)
    b = _gen(tiny_plain, emb)
    assert a[0] == b[0] and len(a[1]) == 20
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    c = _gen(model, emb, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)         # neutral values given explicitly
    assert c[0] == a[0] and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[1], c[1]))
    with pytest.raises(ValueError):
        tiny_plain.generate(inputs_embeds=emb, max_new_tokens=4, repetition_penalty=1.3)
    with pytest.raises(ValueError):
        tiny_plain.generate(inputs_embeds=emb, max_new_tokens=4, output_logprobs=1)


# ---- 5. three sequences in one batched iteration --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from tests import tiny_ckpt
    d = str(tmp_path_factory.mktemp("vita_tiny_rules"))
    tiny_ckpt.write(d, seed=31)
    return d


PROMPTS = [[1, 5, 6, 7, 8], [1, 9, 10, 11, 12, 13, 14, 15], [1, 20, 21]]


def test_batched_sequences_equal_their_solo_runs(ckpt):
    """penalties only, sampling + penalties + logprobs = 20, and plain greedy in flight together (max_num_seqs = 3: the batched LM
    head with per-sequence tables, the filter kernel and the logprob kernel behind it); each equals LLM.generate of the same request
    alone, the plain one the run without rules."""
    from vita_amd.serving import AsyncEngineArgs, AsyncLLMEngine, SamplingParams
    engine = AsyncLLMEngine.from_engine_args(AsyncEngineArgs(model=ckpt, dtype="float16", max_num_seqs=3, max_new_tokens=24,
                                                             kv_pool_tokens=2048, device="cuda:0", max_logprobs=20))
    # negative presence / frequency penalties pull a request onto the tokens it has generated whatever the model's logits are, so a
    # batched path that lost a sequence's table or rules would show in the ids
    sps = [SamplingParams(temperature=0.01, max_tokens=14, repetition_penalty=1.3, frequency_penalty=-2.0, presence_penalty=-2.0),
           SamplingParams(temperature=0.7, top_k=30, top_p=0.9, seed=6, max_tokens=14, repetition_penalty=1.2, frequency_penalty=-2.0,
                          logprobs=20),
           SamplingParams(temperature=0.01, max_tokens=14)]

    async def one(i):
        last = None
        async for out in engine.generate({"prompt_token_ids": PROMPTS[i]}, sampling_params=sps[i], request_id=f"r{i}"):
            last = out.outputs[0]
        return last

    async def main():
        return await asyncio.gather(*[one(i) for i in range(3)])

    got = asyncio.run(main())
    engine.shutdown()
    st = engine.batcher.stats
    # the three really shared iterations: more than two sequences per decode iteration on average needs iterations of width 3
    # (the batched LM head k_decb_lmhead<.., PEN>), and fewer prefill calls than prefills a grouped prefill
    assert st["decode_steps"] > 2 * st["iterations"] and st["prefills"] == 3, st
    assert not engine.batcher.logprobs                                    # finished requests leave nothing behind
    solo = [engine.llm.generate({"prompt_token_ids": PROMPTS[i]}, sampling_params=sps[i])[0].outputs[0] for i in range(3)]
    for i in range(3):
        assert list(got[i].token_ids) == list(solo[i].token_ids), (i, got[i].token_ids, solo[i].token_ids)
    assert got[0].logprobs is None and got[2].logprobs is None and solo[2].logprobs is None
    plain = engine.llm.generate({"prompt_token_ids": PROMPTS[0]}, sampling_params=SamplingParams(temperature=0.01, max_tokens=14))
    assert list(plain[0].outputs[0].token_ids) != list(solo[0].token_ids)                      # the penalties changed request 0
    plain = engine.llm.generate({"prompt_token_ids": PROMPTS[1]}, sampling_params=SamplingParams(temperature=0.7, top_k=30, top_p=0.9,
                                                                                                 seed=6, max_tokens=14))
    assert list(plain[0].outputs[0].token_ids) != list(solo[1].token_ids)                      # and request 1
    a, b = got[1].logprobs, solo[1].logprobs
    assert len(a) == len(b) == len(got[1].token_ids) and all(len(d) >= 20 for d in a)
    worst = 0.0
    for d, e in zip(a, b):
        assert list(d) == list(e), (list(d), list(e))
        ok, w = _ulp_ok([d[k] for k in e], [e[k] for k in e])
        worst = max(worst, w)
    print(f"batched against solo logprobs: worst {worst:.2f} ulp")
    assert worst <= 1.0, worst
    assert abs(got[1].cumulative_logprob - sum(d[t] for d, t in zip(a, got[1].token_ids))) < 1e-6


# ---- 6. recompute preemption ------------------------------------------------------------------------------------------------
def test_recompute_preemption_keeps_ids_and_logprobs(dev):
    """the small-pool set-up of test_batcher_recompute_preemption_keeps_the_draws with a frequency penalty and logprobs: the re-armed
    sequence gets its prompt set and its output counts back, its logprobs run on across the re-prefill.  Ids and logprobs — every
    entry of every token's dict: the top-K ids in order, their values and the chosen id's — are compared with the run that never
    preempts: bit-equal up to a request's first preemption, ids equal and values within 1 ulp after it (see below)."""
    from vita_amd.checkpoint import pack_mixtral
    from vita_amd.engine import MixtralEngine
    from vita_amd.serving import ContinuousBatcher
    cfg = VitaConfig.tiny()
    sd = synth_state_dict(cfg, seed=9, parts=("text",))
    table = torch.from_numpy(sd["model.embed_tokens.weight"]).to(dev)
    rng = np.random.default_rng(16)
    pids = [rng.integers(3, cfg.text.vocab_size, size=S) for S in (60, 62)]
    embs = [table[torch.from_numpy(p).to(dev)] for p in pids]
    samp = [dict(temperature=1.1, top_k=0, top_p=1.0, seed=41), dict(temperature=0.9, top_k=25, top_p=0.9, seed=42)]
    rules = [dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.7, logprobs=5),
             dict(repetition_penalty=1.2, presence_penalty=0.3, frequency_penalty=0.7, logprobs=3)]
    n_new = 80
    runs = []
    for pool in (256, 1024):
        eng = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev), dev, max_ctx=pool, max_prefill=160, max_new=n_new + 4, max_seqs=2,
                            penalty_tables=True, max_logprobs=5)
        bt = ContinuousBatcher(eng, embed_tokens=lambda ids: table[ids], window=4)
        for i, e in enumerate(embs):
            bt.add(i, e, max_tokens=n_new, sampling=samp[i], rules=rules[i], prompt_ids=pids[i].tolist())
        got, first_cut = {}, {}
        for _ in range(10000):
            if not bt.has_work():
                break
            for rid, new, finished, reason in bt.step():
                got.setdefault(rid, []).extend(new)
            for r in bt.waiting:                      # a preempted request waits with base = tokens it had generated
                first_cut.setdefault(r.id, r.base)
        assert all(len(got[i]) == n_new for i in range(2)), {i: len(v) for i, v in got.items()}
        runs.append((got, bt.stats["preemptions"], {i: list(bt.logprobs[i]) for i in range(2)}, first_cut))
        eng.close()
    (small, npre, lp_s, cuts), (big, nbig, lp_b, _) = runs
    assert npre >= 1 and nbig == 0 and cuts and all(0 < c < n_new for c in cuts.values()), (npre, nbig, cuts)
    assert small == big
    # Everything a request produced BEFORE its first preemption (all of it for a request that never yields) is bit-equal: the same
    # kernels ran on the same state.  After a re-prefill the K / V rows of the tokens generated so far were written by the prefill
    # kernels instead of the decode kernels, so the scores are those of another code path: the ids still have to be equal entry by
    # entry and in order, the values are held to the bound the contract sets for a sequence's logprobs across two code paths
    # (batched against solo: 1 fp32 ulp), for all K + 1 entries.  Measured: no id differs, worst 1.00 ulp after the cut, 0 before.
    worst_pre, worst_post = 0.0, 0.0
    for i in range(2):
        assert len(lp_s[i]) == len(lp_b[i]) == n_new
        cut = cuts.get(i, n_new)
        for j, (t, d, e) in enumerate(zip(small[i], lp_s[i], lp_b[i])):
            K = rules[i]["logprobs"]
            assert t in d and K <= len(d) <= K + 1
            assert list(d) == list(e), (i, j, list(d), list(e))                    # the top-K ids in order, then the chosen id
            w = max(abs(d[k] - e[k]) / float(np.spacing(np.float32(abs(e[k])))) for k in e)
            if j < cut:
                worst_pre = max(worst_pre, w)
            else:
                worst_post = max(worst_post, w)
    print(f"preempted at {cuts}; against the unpreempted run: worst {worst_pre:.2f} ulp before the cut, {worst_post:.2f} ulp after")
    assert worst_pre == 0.0, worst_pre
    assert worst_post <= 1.0, worst_post


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_setters_refuse_and_keep_the_previous_setting(dev):
    from vita_amd._lib import VitaHipError
    from vita_amd.checkpoint import pack_mixtral
    from vita_amd.engine import MixtralEngine
    cfg = VitaConfig.tiny()
    V = cfg.text.vocab_size
    sd = synth_state_dict(cfg, seed=2, parts=("text",))
    kw = dict(max_ctx=256, max_prefill=64, max_new=8)
    refused = lambda what: pytest.raises(VitaHipError, match=what + r" failed \(rc=-2\)")
    plain = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev), dev, max_seqs=2, **kw)              # created without tables
    try:
        with refused("vh_mixtral_set_logit_rules"):
            plain.set_logit_rules(1.3)
        with refused("vh_mixtral_set_logit_rules"):
            plain.set_logit_rules()
        with refused("vh_mixtral_seq_set_logit_rules"):
            plain.seq_set_logit_rules(plain.seq_alloc(), logprobs=1)
        with pytest.raises(VitaHipError):
            plain.logprobs()
    finally:
        plain.close()
    shard = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev, rank=0, world=2, shard_vocab=True), dev, rank=0, world=2,
                          penalty_tables=True, max_logprobs=5, **kw)                             # vocab-sharded head
    try:
        assert shard.c.vocab_n > 0
        with refused("vh_mixtral_set_logit_rules"):
            shard.set_logit_rules(1.3)
        with refused("vh_mixtral_set_logit_rules"):
            shard.set_logit_rules(logprobs=0)
        shard.set_logit_rules()                                                               # "off" stays acceptable
    finally:
        shard.close()
    eng = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev), dev, max_seqs=2, logit_rows=8, penalty_tables=True, max_logprobs=5, **kw)
    try:
        s = eng.seq_alloc()
        prompt = [5, 6, 7, 7]
        eng.seq_set_logit_rules(s, 1.3, 0.4, 0.6, 3, prompt_ids=prompt, output_ids=[9, 9])
        eng.set_logit_rules(1.3, 0.4, 0.6, 3, prompt_ids=prompt, output_ids=[9, 9])
        before = (eng.seen_table().cpu().numpy().copy(), eng.seen_table(s).cpu().numpy().copy())
        assert np.array_equal(before[0].view(np.uint32), ref.seen_table(V, prompt, [9, 9]))
        assert np.array_equal(before[1].view(np.uint32), ref.seen_table(V, prompt, [9, 9]))
        bad = [dict(prompt_ids=[V]), dict(prompt_ids=[1], output_ids=[-1]), dict(logprobs=6), dict(logprobs=-2),
               dict(repetition_penalty=0.0), dict(repetition_penalty=float("nan")), dict(presence_penalty=float("inf")),
               dict(frequency_penalty=float("nan"))]
        for b in bad:
            with refused("vh_mixtral_set_logit_rules"):
                eng.set_logit_rules(**b)
            with refused("vh_mixtral_seq_set_logit_rules"):
                eng.seq_set_logit_rules(s, **b)
        with refused("vh_mixtral_seq_set_logit_rules"):
            eng.seq_set_logit_rules(1 - s, 1.3)                                                # a dead slot
        with refused("vh_mixtral_seq_set_logit_rules"):
            eng.seq_set_logit_rules(7, 1.3)
        after = (eng.seen_table().cpu().numpy(), eng.seen_table(s).cpu().numpy())
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        # the previous setting is still in force: a short run obeys it (single-sequence engine, scores kept)
        eng.seq_free(s)
        emb = torch.from_numpy(sd["model.embed_tokens.weight"][np.random.default_rng(5).integers(3, V, size=20)]).to(dev).float()
        eng.prefill(emb)
        eng.decode(4)
        torch.cuda.synchronize()
        ids = eng.generated()
        scores = [eng.logits_all[i].cpu().numpy() for i in range(5)]
        hist = [9, 9] + ids
        exp = [int(np.argmax(ref.penalise(scores[i], ref.seen_table(V, prompt, hist[:2 + i]), r=1.3, f=0.6, p=0.4))) for i in range(5)]
        assert ids == exp, (ids, exp)
        tok, top_id, top = eng.logprobs()
        for i in range(5):
            e_lp, e_ids, e_top = ref.logprobs(scores[i], ids[i], 3)
            assert top_id[i, :3].tolist() == e_ids.tolist()
            assert _ulp_ok(tok[i:i + 1].cpu().numpy(), [e_lp])[0] and _ulp_ok(top[i, :3].cpu().numpy(), e_top)[0]
        eng.reset()                                                                            # reset restores "off"
        eng.prefill(emb)
        eng.decode(4)
        torch.cuda.synchronize()
        assert eng.generated() == [int(np.argmax(eng.logits_all[i].cpu().numpy())) for i in range(5)]
        # a call without penalties clears the history an earlier request left in the table
        assert int((eng.seen_table() != 0).sum().item()) > 0
        eng.set_logit_rules(logprobs=1)
        assert int((eng.seen_table() != 0).sum().item()) == 0
        eng.set_logit_rules(1.3, prompt_ids=[5])
        eng.set_logit_rules()
        assert int((eng.seen_table() != 0).sum().item()) == 0
        with pytest.raises(VitaHipError):
            eng.logprobs(99)                                                                   # no such slot
        with pytest.raises(VitaHipError):
            eng.seen_table(-1)
    finally:
        eng.close()
