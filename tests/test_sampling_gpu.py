"""Seeded temperature / top-k / top-p sampling on the device (vh_sample.h) against its numpy restatement (tests/sampling_ref.py):
the RNG pinned to numpy's Philox, every token of the filter kernel equal to the restatement, the draw distribution, degenerate
rows, the engine's generate() across lookahead windows, and the serving surfaces (LLM, AsyncLLMEngine, recompute preemption)."""
import asyncio

import numpy as np
import pytest
import torch

from tests import sampling_ref as ref
from tests.ranks import run_ranks
from vita_amd import ops
from vita_amd.checkpoint import synth_state_dict
from vita_amd.config import VitaConfig

pytestmark = pytest.mark.gpu


def _dev_ids(logits_np, rows=None, **kw):
    t = torch.from_numpy(np.ascontiguousarray(logits_np, dtype=np.float32)).cuda()
    out = ops.sample_rows(t, rows=rows, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_rng_pinned_to_numpy_philox():
    """all-zero logits, V = 4, T = 1: the token is the argmax of the four Philox words of block (0, draw) — numpy's Philox,
    which increments its counter before each block."""
    seed, n = 20241022, 4096
    got = _dev_ids(np.zeros(4, np.float32), rows=n, temperature=1.0, seed=seed)
    exp = []
    for d in range(n):
        c = (d << 64) - 1                          # counter (0, d, 0, 0) minus one, borrow across words
        words = np.random.Philox(key=seed, counter=c % (1 << 256)).random_raw(4)
        exp.append(int(np.argmax(words >> np.uint64(11))))
    assert got.tolist() == exp


@pytest.mark.parametrize("V", [1000, 32002, 51760])
def test_filter_kernel_equals_the_restatement(V):
    rng = np.random.default_rng(V)
    rows = np.stack([(rng.standard_normal(V) * 2.5).astype(np.float32) for _ in range(3)])
    rows[1, rng.integers(0, V, 40)] = rows[1].max()                    # tied maxima
    rows[2] = np.round(rows[2] * 4) / 4                                # many ties everywhere
    bad = []
    n = 0
    for T in (0.01, 0.7, 1.0, 1.5):
        for top_k in (0, 1, 5, 50, V):
            for top_p in (1.0, 0.95, 0.5, 1e-6):
                seed = (V * 7919 + n) & 0xFFFFFFFF
                got = _dev_ids(rows, temperature=T, top_k=top_k, top_p=top_p, seed=seed, draw0=100 * n)
                for r in range(rows.shape[0]):
                    exp = ref.sample(rows[r], T, top_k, top_p, seed, 100 * n + r)
                    if int(got[r]) != exp:
                        bad.append((T, top_k, top_p, r, int(got[r]), exp, ref.top2_gap(rows[r], T, top_k, top_p, seed, 100 * n + r)))
                n += 1
    assert not bad, f"{len(bad)} tokens differ (T, top_k, top_p, row, device, host, host top-2 perturbed gap): {bad[:8]}"


def test_draw_distribution_chi_square():
    """2^20 draws of one V = 64 row at T = 0.7, top_k = 20, top_p = 0.9 against the exact filtered softmax (fixed seed: the
    statistic is a fixed number)."""
    rng = np.random.default_rng(3)
    row = (rng.standard_normal(64) * 0.6).astype(np.float32)     # top-k cuts 44 tokens, top-p 3 more: 17 kept
    n = 1 << 20
    got = _dev_ids(row, rows=n, temperature=0.7, top_k=20, top_p=0.9, seed=99)
    p = ref.filtered_softmax(row, 0.7, 20, 0.9)
    counts = np.bincount(got, minlength=64)
    assert counts[p == 0].sum() == 0, "a filtered token was drawn"
    keep = p > 0
    exp = p[keep] * n
    chi2 = float(((counts[keep] - exp) ** 2 / exp).sum())
    dof = int(keep.sum()) - 1
    # 99.9 % quantile of chi2(dof) (Wilson-Hilferty), 16 degrees of freedom here
    z = 3.09
    q = dof * (1 - 2 / (9 * dof) + z * np.sqrt(2 / (9 * dof))) ** 3
    assert 5 <= dof <= 20 and chi2 < q, (chi2, dof, q)


def test_degenerate_rows():
    rng = np.random.default_rng(11)
    for V in (1, 3, 7, 1001, 51759):
        row = rng.standard_normal(V).astype(np.float32)
        greedy = int(np.argmax(row))
        assert _dev_ids(row, rows=8, temperature=0.9, top_k=1, seed=5).tolist() == [greedy] * 8
        assert _dev_ids(row, rows=8, temperature=0.9, top_p=1e-6, seed=5).tolist() == [greedy] * 8
        assert _dev_ids(row, rows=2, temperature=0.0, seed=5).tolist() == [greedy] * 2
        got = _dev_ids(row, rows=64, temperature=1.3, top_k=3, top_p=0.8, seed=6)
        assert ((0 <= got) & (got < V)).all()
        assert got.tolist() == [ref.sample(row, 1.3, 3, 0.8, 6, d) for d in range(64)]
    for fill in (np.nan, -np.inf):
        row = np.full(1003, fill, np.float32)
        for kw in (dict(), dict(top_k=5), dict(top_p=0.5)):
            got = _dev_ids(row, rows=4, temperature=1.0, seed=1, **kw)
            assert ((0 <= got) & (got < 1003)).all() and got.tolist() == [0] * 4
        row[[17, 600]] = [1.0, 2.0]                                        # two finite entries among NaN / -inf
        got = _dev_ids(row, rows=32, temperature=1.0, top_p=0.9, seed=2)
        assert got.tolist() == [ref.sample(row, 1.0, 0, 0.9, 2, d) for d in range(32)]


BAD_ARGS = (dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(top_k=-1),
            dict(top_p=0.0), dict(top_p=1.5))


def test_invalid_arguments_raise():
    from vita_amd._lib import VitaHipError
    t = torch.zeros(8, device="cuda")
    for kw in BAD_ARGS:
        with pytest.raises(VitaHipError, match=r"vh_sample_rows failed \(rc=-2\)"):
            ops.sample_rows(t, rows=1, **kw)


def test_engine_sampling_arguments_are_checked(dev):
    """vh_mixtral_set_sampling / vh_mixtral_seq_set_sampling refuse what vh_sample_rows refuses (VH_E_ARG), and a sequence
    slot that is not allocated; a refused call leaves the previous setting in force."""
    from vita_amd._lib import VitaHipError
    from vita_amd.checkpoint import pack_mixtral
    from vita_amd.engine import MixtralEngine
    cfg = VitaConfig.tiny()
    sd = synth_state_dict(cfg, seed=2, parts=("text",))
    eng = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev), dev, max_ctx=256, max_prefill=64, max_new=8, max_seqs=2)
    try:
        s = eng.seq_alloc()
        for kw in BAD_ARGS:
            with pytest.raises(VitaHipError, match=r"vh_mixtral_set_sampling failed \(rc=-2\)"):
                eng.set_sampling(**kw)
            with pytest.raises(VitaHipError, match=r"vh_mixtral_seq_set_sampling failed \(rc=-2\)"):
                eng.seq_set_sampling(s, **kw)
        with pytest.raises(VitaHipError, match=r"rc=-2"):
            eng.seq_set_sampling(1 - s, temperature=1.0)          # not allocated
        eng.seq_set_sampling(s, temperature=0.5, top_k=3, seed=4)    # valid settings are accepted
        eng.set_sampling(temperature=0.0)
    finally:
        eng.close()


# ---- engine ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(dev):
    from vita_amd.model import build_synthetic_model
    model, sd = build_synthetic_model(VitaConfig.tiny(), seed=17, device=dev, max_new_tokens=32, max_prefill=512)
    rng = np.random.default_rng(4)
    ids = rng.integers(3, VitaConfig.tiny().text.vocab_size, size=37)
    emb = torch.from_numpy(sd["model.embed_tokens.weight"][ids]).to(dev)[None].float()
    return model, emb


def _gen(model, emb, n=20, **kw):
    out = model.generate(inputs_embeds=emb, max_new_tokens=n, eos_token_id=-1, return_dict_in_generate=True, output_scores=True, **kw)
    torch.cuda.synchronize()
    return out.sequences[0].tolist(), [s[0].cpu().numpy() for s in out.scores]


@pytest.mark.parametrize("params", [dict(temperature=1.3, top_k=0, top_p=1.0), dict(temperature=0.8, top_k=12, top_p=0.9),
                                    dict(temperature=1.0)])   # the last: HF defaults top_k 50, top_p 1
def test_engine_generate_samples_the_contract(tiny, params):
    model, emb = tiny
    greedy0, _ = _gen(model, emb)
    ids, scores = _gen(model, emb, do_sample=True, seed=1234, **params)
    assert len(ids) == 20 and len(scores) == 20                      # crosses two lookahead windows of 8
    T, k, p = params["temperature"], params.get("top_k", 50), params.get("top_p", 1.0)
    exp = [ref.sample(scores[i], T, k, p, 1234, i) for i in range(20)]
    assert ids == exp, (ids, exp)
    assert _gen(model, emb, do_sample=True, seed=1234, **params)[0] == ids
    assert _gen(model, emb, do_sample=True, seed=99, **params)[0] != ids
    assert ids != greedy0
    assert _gen(model, emb)[0] == greedy0                            # greedy again afterwards
    with pytest.raises(NotImplementedError):
        model.generate(inputs_embeds=emb, max_new_tokens=4, do_sample=True, temperature=1.0)
    with pytest.raises(ValueError):                                  # HF refuses do_sample with temperature 0 too
        model.generate(inputs_embeds=emb, max_new_tokens=4, do_sample=True, temperature=0.0, seed=1)


# ---- serving --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from tests import tiny_ckpt
    d = str(tmp_path_factory.mktemp("vita_tiny_sampling"))
    tiny_ckpt.write(d, seed=31)
    return d


PROMPTS = [[1, 5, 6, 7, 8], [1, 9, 10, 11, 12, 13, 14, 15], [1, 20, 21]]


def test_llm_generate_equals_model_generate(ckpt, dev):
    from vita_amd.serving import LLM, SamplingParams
    llm = LLM(model=ckpt, dtype="float16", tensor_parallel_size=1, max_new_tokens=24)
    sp = SamplingParams(temperature=0.9, top_k=-1, top_p=0.95, seed=7, max_tokens=12)
    got = llm.generate({"prompt_token_ids": PROMPTS[0]}, sampling_params=sp)[0].outputs[0].token_ids
    req = llm._prepare({"prompt_token_ids": PROMPTS[0]}, sp)
    emb = llm._embed(req)
    out = llm.model.generate(inputs_embeds=emb[None], max_new_tokens=12, do_sample=True, temperature=0.9, top_k=0, top_p=0.95,
                             seed=7, eos_token_id=list(req["eos"]))
    assert got == out[0].tolist() and len(got) >= 1
    greedy = llm.generate({"prompt_token_ids": PROMPTS[0]}, sampling_params=SamplingParams(max_tokens=12))[0].outputs[0].token_ids
    assert got != greedy
    with pytest.raises(NotImplementedError):
        llm.generate({"prompt_token_ids": PROMPTS[0]}, sampling_params=SamplingParams(temperature=0.8))


def test_async_engine_sampled_requests_equal_their_solo_runs(ckpt):
    """two sampled requests (different parameters) and one greedy, in flight together (max_num_seqs = 3: the batched LM head
    with per-sequence sampling and the filter kernel behind it); each equals LLM.generate of the same request alone."""
    from vita_amd.serving import AsyncEngineArgs, AsyncLLMEngine, SamplingParams
    engine = AsyncLLMEngine.from_engine_args(AsyncEngineArgs(model=ckpt, dtype="float16", max_num_seqs=3, max_new_tokens=24,
                                                             kv_pool_tokens=2048, device="cuda:0"))
    sps = [SamplingParams(temperature=1.2, top_k=-1, seed=5, max_tokens=14), SamplingParams(temperature=0.7, top_k=30, top_p=0.9,
                                                                                             seed=6, max_tokens=14),
           SamplingParams(temperature=0.01, max_tokens=14)]

    async def one(i):
        last = None
        async for out in engine.generate({"prompt_token_ids": PROMPTS[i]}, sampling_params=sps[i], request_id=f"s{i}"):
            last = list(out.outputs[0].token_ids)
        return last

    async def main():
        return await asyncio.gather(*[one(i) for i in range(3)])

    got = asyncio.run(main())
    engine.shutdown()
    for i in range(3):
        exp = engine.llm.generate({"prompt_token_ids": PROMPTS[i]}, sampling_params=sps[i])[0].outputs[0].token_ids
        assert got[i] == exp, (i, got[i], exp)


def test_batcher_recompute_preemption_keeps_the_draws(dev):
    """a pool small enough to preempt (4 pages, two sequences growing past 128 tokens): the sampled ids equal the run with a pool
    that never preempts — the re-armed sequence continues at draw0 = tokens already generated."""
    from vita_amd.checkpoint import pack_mixtral
    from vita_amd.engine import MixtralEngine
    from vita_amd.serving import ContinuousBatcher
    cfg = VitaConfig.tiny()
    sd = synth_state_dict(cfg, seed=9, parts=("text",))
    table = torch.from_numpy(sd["model.embed_tokens.weight"]).to(dev)
    rng = np.random.default_rng(16)
    embs = [table[torch.from_numpy(rng.integers(3, cfg.text.vocab_size, size=S)).to(dev)] for S in (60, 62)]
    samp = [dict(temperature=1.1, top_k=0, top_p=1.0, seed=41), dict(temperature=0.9, top_k=25, top_p=0.9, seed=42)]
    n_new = 80
    runs = []
    for pool in (256, 1024):
        eng = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev), dev, max_ctx=pool, max_prefill=160, max_new=n_new + 4, max_seqs=2)
        bt = ContinuousBatcher(eng, embed_tokens=lambda ids: table[ids], window=4)
        for i, e in enumerate(embs):
            bt.add(i, e, max_tokens=n_new, sampling=samp[i])
        got = {}
        for _ in range(10000):
            if not bt.has_work():
                break
            for rid, new, finished, reason in bt.step():
                got.setdefault(rid, []).extend(new)
        assert all(len(got[i]) == n_new for i in range(2)), {i: len(v) for i, v in got.items()}
        runs.append((got, bt.stats["preemptions"]))
        eng.close()
    (small, npre), (big, nbig) = runs
    assert npre >= 1 and nbig == 0
    assert small == big


# ---- tensor parallel: two engine processes on one GPU (the pattern of tests/test_comm_gpu.py) ---------------------------------
TP_MODES = {"temperature": dict(temperature=1.2, top_k=0, top_p=1.0, seed=77),
            "top_p": dict(temperature=0.9, top_k=0, top_p=0.8, seed=78)}


def _tp_sampling_worker(ctx, shard_vocab):
    import torch.distributed as dist
    from vita_amd._lib import VitaHipError
    from vita_amd.checkpoint import pack_mixtral
    from vita_amd.engine import MixtralEngine
    from vita_amd.parallel import setup_tensor_parallel
    rank, world, dev = ctx.rank, ctx.world, ctx.dev
    cfg = VitaConfig.tiny()
    sd = synth_state_dict(cfg, seed=3, parts=("text",))
    packed = pack_mixtral(sd, cfg, dev, rank=rank, world=world, shard_vocab=shard_vocab)
    eng = MixtralEngine(cfg, packed, dev, max_ctx=128, max_prefill=64, max_new=16, rank=rank, world=world, logit_rows=16)
    ctx.defer(eng.close)
    name = setup_tensor_parallel(eng, rank, world, dev, backend="gloo", collective="ipc")
    ids = np.random.default_rng(5).integers(3, cfg.text.vocab_size, size=37).tolist()
    emb = packed["embed"][torch.as_tensor(ids, device=dev)].float()
    out = {"collective": name, "sharded": eng.vocab_sharded}
    for mode, kw in TP_MODES.items():
        try:
            eng.set_sampling(**kw)
        except VitaHipError as e:
            out[mode] = ("raised", str(e))
            continue
        eng.prefill(emb)
        eng.decode(11)
        torch.cuda.synchronize()
        lg = eng.logits_all[:12].cpu()
        if eng.vocab_sharded:
            dist.all_reduce(lg)              # a kept row holds this rank's slice and zeros elsewhere
        out[mode] = (eng.generated(), lg.numpy())
    eng.set_sampling()
    return out


def _check_draws(r0, r1, mode):
    kw = TP_MODES[mode]
    ids0, lg0 = r0[mode]
    ids1, lg1 = r1[mode]
    assert ids0 == ids1 and len(ids0) == 12, (ids0, ids1)
    assert np.array_equal(lg0, lg1)
    exp = [ref.sample(lg0[i], kw["temperature"], kw["top_k"], kw["top_p"], kw["seed"], i) for i in range(12)]
    assert ids0 == exp, (mode, ids0, exp)


def test_tp2_vocab_sharded_head_samples_temperature_only_and_refuses_filters():
    """sharded head: each rank draws over its slice (global vocab indices), the exact candidates travel through the all-reduce,
    both ranks emit the same ids — the restatement's on the gathered rows; top-p is refused (VH_E_ARG)."""
    r0, r1 = run_ranks(_tp_sampling_worker, 2, True, deadline_s=120)
    assert r0["collective"] == r1["collective"] == "ipc" and r0["sharded"] and r1["sharded"]
    _check_draws(r0, r1, "temperature")
    for r in (r0, r1):
        assert r["top_p"][0] == "raised" and "rc=-2" in r["top_p"][1], r["top_p"]


def test_tp2_unsharded_head_draws_the_same_token_on_every_rank():
    """unsharded head under TP: every rank holds the same logits and draws the same token, temperature-only and top-p."""
    r0, r1 = run_ranks(_tp_sampling_worker, 2, False, deadline_s=120)
    assert r0["collective"] == r1["collective"] == "ipc" and not r0["sharded"] and not r1["sharded"]
    _check_draws(r0, r1, "temperature")
    _check_draws(r0, r1, "top_p")
