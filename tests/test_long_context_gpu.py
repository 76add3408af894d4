"""The text backbone past 4096 tokens: the range a 16-frame video prompt reaches (16 x 256 image tokens + text + audio ~ 4 400 rows;
the released model takes prompts up to tokenizer_model_max_length = 4600, vita_amd/config.py).  Several kernels change path there:

  k_moe_sort          2S > 8192 (S > 4096): the (token, slot) ids are staged in LDS in chunks, two passes with reloads;
  k_attn_fa<1, true, 2>  the image-tile 32-row flash form at 72 key tiles with a 56-key last tile (the engine's default at S = 4600);
  dec_attn_finish     decode at pos >= 4096: more than 64 splits, the merge runs a second round of 64 lanes (k_dec_attn, k_dec_ablk);
  page tables         a served sequence of more than 64 pages: chunked prefill through the table, batched decode.

Against the fp32 oracle (oracle/mixtral.py) with the bars of tests/test_mixtral_gpu.py: per-layer prefill hidden states within
3e-4 of the tensor's largest magnitude + 1e-3 relative, every logit row within 1e-3, greedy ids and every router decision equal.
The oracle takes the ENGINE's RoPE rows (a test-local patch of om.rope_cos_sin): the two tables compute inv_freq in different orders
and differ by one fp32 ulp of the angle, up to 4.9e-4 on cos / sin past 4096 — no bit-exact target exists, and the kernels, not the
table definitions, are under test.  Router decisions and greedy ids are discontinuous: each test asserts that the oracle's smallest
margin (2nd - 3rd router logit of every decision, top-1 - top-2 logit of every greedy step) is clear of the error (> MARGIN), so a
failure is a wrong kernel and never a tie; the seeds were chosen for that."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import mixtral as om
from tests.seq_scores import check_sequence
from tests.util import assert_close, to_np
from vita_amd.checkpoint import pack_mixtral, round_bf16, synth_state_dict
from vita_amd.config import TextConfig, VitaConfig
from vita_amd.engine import rope_tables

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3
MARGIN = 1e-4          # smallest oracle margin a discontinuous decision may have (errors of the compared quantities: ~1e-5)
S_LIMIT = 4600         # tokenizer_model_max_length


def _cfg(layers, hidden=1024, nq=32, nkv=8):
    """the released attention geometry (32 : 8 heads of 128: image tiles, 32-row flash form, XCD pairs and G = 4 decode are what the
    engine picks by itself) with an MoE and projections small enough for the numpy oracle at S = 4600."""
    cfg = VitaConfig.tiny()
    cfg.text = TextConfig(hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=nq, num_key_value_heads=nkv, head_dim=128,
                          intermediate_size=1024, num_local_experts=8, vocab_size=2000)
    return cfg


@contextlib.contextmanager
def _oracle_patches(t, max_pos):
    """om.rope_cos_sin -> the engine's rows; om.moe also records the smallest 2nd - 3rd router logit margin of every call."""
    cos, sin = rope_tables(max_pos, t.head_dim, t.rope_theta)
    margins = []
    moe = om.moe

    def rope(positions, head_dim, theta):
        p = np.asarray(positions)
        return np.concatenate([cos[p], cos[p]], -1), np.concatenate([sin[p], sin[p]], -1)

    def moe_margin(x, lw, top_k=2, force=None):
        lg = np.sort((x @ lw["gate"].T).astype(np.float32), -1)
        margins.append(float((lg[:, -2] - lg[:, -3]).min()))
        return moe(x, lw, top_k, force)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(om, "rope_cos_sin", rope)
        mp.setattr(om, "moe", moe_margin)
        yield margins


def _oracle(sd, t, emb, n_steps):
    """one oracle pass: prefill (hidden states after every layer, sorted top-2 expert pairs of every row and layer) and n_steps greedy
    score rows; margins of every router decision (prefill and decode) and of every greedy pick."""
    with _oracle_patches(t, emb.shape[0] + n_steps + 8) as margins:
        orc = om.MixtralOracle(sd, t)
        lg, hid = orc.forward(emb, want_hidden=True)
        route = np.stack([np.sort(idx, -1) for idx, _ in orc.last_route])
        ids, rows = [], []
        for i in range(n_steps):
            rows.append(lg[-1].copy())
            ids.append(int(np.argmax(lg[-1])))
            if i + 1 < n_steps:
                lg, _ = orc.forward(orc.embed[ids[-1]][None])
    rows = np.stack(rows)
    top = np.sort(rows, -1)
    return dict(ids=ids, logits=rows, hid=hid, route=route, router_margin=min(margins),
                logit_margin=float((top[:, -1] - top[:, -2]).min()))


def _assert_margins(ref):
    print(f"oracle margins: router {ref['router_margin']:.2e}, greedy logits {ref['logit_margin']:.2e}")
    assert ref["router_margin"] > MARGIN, "a router decision of the oracle is a tie: choose another seed"
    assert ref["logit_margin"] > MARGIN, "a greedy pick of the oracle is a tie: choose another seed"


def _check_engine(dev, cfg, sd, emb, ref, n_new, schedule=None):
    """one-shot prefill (hidden states, routing) + n_new - 1 decode steps in one call against the oracle pass."""
    from vita_amd.engine import MixtralEngine
    S, L = emb.shape[0], cfg.text.num_hidden_layers
    eng = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev), dev, max_ctx=S + n_new + 8, max_prefill=S, max_new=n_new + 4,
                        logit_rows=n_new + 4)
    try:
        _, hid = eng.prefill(torch.from_numpy(emb).to(dev), want_hidden=True, want_route=True)
        route = np.sort(eng.route_ids.cpu().numpy(), -1)
        for l in range(L):
            assert_close(f"prefill hidden after layer {l} (S = {S})", to_np(hid[l]), ref["hid"][l],
                         atol=3e-4 * float(np.abs(ref["hid"][l]).max()), rtol=1e-3)
            bad = np.flatnonzero((route[l] != ref["route"][l]).any(-1))
            assert bad.size == 0, f"layer {l}: {bad.size} router decisions differ from the oracle, first at rows {bad[:8].tolist()}"
        del hid
        if n_new > 1:
            eng.decode(n_new - 1)
        torch.cuda.synchronize()
        if schedule is not None:
            assert eng.decode_schedule() == schedule
        for i in range(n_new):
            assert_close(f"logits step {i} (position {S + i - 1})", to_np(eng.logits_all[i]), ref["logits"][i], atol=LOGIT_TOL)
        got = eng.generated()
        print("oracle ids:", ref["ids"], "device ids:", got)
        assert got == ref["ids"], "greedy token ids differ from the oracle"
        assert int(eng.counters[0].item()) == S + n_new - 1
    finally:
        eng.close()


# ---- a. a prompt at the model's limit ------------------------------------------------------------------------------------------
LIMIT_SEED, LIMIT_STEPS = 1, 8


@pytest.fixture(scope="module")
def limit_prompt():
    cfg = _cfg(2)
    sd = synth_state_dict(cfg, seed=LIMIT_SEED, parts=("text",))
    ids = np.random.default_rng(LIMIT_SEED + 100).integers(3, cfg.text.vocab_size, size=S_LIMIT)
    emb = sd["model.embed_tokens.weight"][ids]
    return cfg, sd, emb, _oracle(sd, cfg.text, emb, LIMIT_STEPS)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fused", [1, 0], ids=["one-launch-block", "three-launches"])
def test_prompt_at_model_limit(dev, limit_prompt, fused):
    """S = 4600, two layers (layer 1 consumes layer 0's pending fused combine), 8 greedy steps: the chunked k_moe_sort (2S = 9200 ids),
    the image-tile 32-row flash form at 72 key tiles, and decode at positions 4600 ... 4606 — 72 splits, a second merge round
    (73 splits: tests/test_ops_gpu.py test_attn_decode_long_context at pos 4671) — in both forms of the decode attention block (dec_fused 1: k_dec_ablk, one launch; 0: k_dec_attn, three launches)."""
    from vita_amd import _lib
    cfg, sd, emb, ref = limit_prompt
    _assert_margins(ref)
    _lib.tune("dec_fused", fused)
    try:
        _check_engine(dev, cfg, sd, emb, ref, LIMIT_STEPS, schedule="fused-attention-block" if fused else "three-launches")
    finally:
        _lib.tune("dec_fused", -1)


# ---- b. skewed routing: a static scene ----------------------------------------------------------------------------------------
SKEW_SEED, SKEW_STEPS = 2, 2


@pytest.mark.timeout(600)
def test_prompt_at_model_limit_skewed_routing(dev):
    """A static video scene sends most rows to the same experts.  A shared direction u is added to every embedding row and router
    rows 0 and 1 are pulled towards u, so that >= 90 % of the 2S = 9200 (token, slot) entries land on experts 0 and 1: one expert holds
    thousands of rows — many balanced m-tiles of the streaming GEMM and a K split chosen on the device — while the others hold few.
    One layer (the suite's time budget; the two-layer hand-over is case a)."""
    cfg = _cfg(1)
    t = cfg.text
    sd = synth_state_dict(cfg, seed=SKEW_SEED, parts=("text",))
    rng = np.random.default_rng(SKEW_SEED + 100)
    u = rng.standard_normal(t.hidden_size)
    u /= np.linalg.norm(u)
    g = sd["model.layers.0.block_sparse_moe.gate.weight"]
    g[:2] = round_bf16((g[:2] + 0.25 * u[None, :]).astype(np.float32))
    ids = rng.integers(3, t.vocab_size, size=S_LIMIT)
    emb = (sd["model.embed_tokens.weight"][ids] + 2.0 * np.sqrt(t.hidden_size) * u[None, :]).astype(np.float32)
    ref = _oracle(sd, t, emb, SKEW_STEPS)
    _assert_margins(ref)
    share = float(np.isin(ref["route"][0], [0, 1]).mean())
    print(f"share of the (token, slot) entries on experts 0 and 1: {share:.4f}")
    assert share >= 0.9
    _check_engine(dev, cfg, sd, emb, ref, SKEW_STEPS)


# ---- c. a served sequence of more than 64 pages ------------------------------------------------------------------------------
PAGED_SEED, PAGED_STEPS, PAGED_CHUNK, PAGED_LOGPROBS = 9, 10, 2048, 20


@pytest.mark.timeout(600)
def test_paged_sequence_past_64_pages(dev):
    """Two sequences of 4200 and 37 tokens on the paged KV cache (8 : 2 heads, hidden 512: the geometry of test_group4_experts8).  The
    long one is prefilled in chunks of max_prefill = 2048 (the flash form through the page table, k_rope_kv with `table`) with the
    short one's prefill in between, so that its 66 pages are not contiguous; then both advance together through the batched decode
    kernels.  Ids equal each request's own oracle; the prefill score rows, and the row a one-token prefill at position 4209 takes
    from K / V rows written by the decode steps, within 1e-3.  Every batched step's scores: both sequences keep logprobs = 20, and
    every generated token's log-probability and top-20 list are held to the oracle's row of that step within 2 LOGIT_TOL
    (tests/seq_scores.py) — 66 splits next to 1 in one k_decb_attn launch, the second lane round of its merge."""
    from vita_amd.engine import MixtralEngine
    cfg = _cfg(2, hidden=512, nq=8, nkv=2)
    t = cfg.text
    lens = (4200, 37)
    sd = synth_state_dict(cfg, seed=PAGED_SEED, parts=("text",))
    rng = np.random.default_rng(PAGED_SEED + 7)
    embs, refs = [], []
    for S in lens:
        emb = sd["model.embed_tokens.weight"][rng.integers(3, t.vocab_size, size=S)]
        embs.append(torch.from_numpy(emb).to(dev))
        refs.append(_oracle(sd, t, emb, PAGED_STEPS + 1))
        _assert_margins(refs[-1])
    pool = 70 * 64                       # 66 + 1 pages are needed
    eng = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev), dev, max_ctx=pool, max_prefill=PAGED_CHUNK, max_new=PAGED_STEPS + 4,
                        max_seqs=2, max_logprobs=PAGED_LOGPROBS)
    try:
        a, b = eng.seq_alloc(), eng.seq_alloc()
        eng.seq_set_logit_rules(a, logprobs=PAGED_LOGPROBS)
        eng.seq_set_logit_rules(b, logprobs=PAGED_LOGPROBS)
        A, B = embs
        eng.seq_prefill(a, A[:PAGED_CHUNK])
        lg_b = eng.seq_prefill(b, B, want_logits=True)              # B's page lands between A's
        eng.seq_prefill(a, A[PAGED_CHUNK:2 * PAGED_CHUNK])
        lg_a = eng.seq_prefill(a, A[2 * PAGED_CHUNK:], want_logits=True)
        assert_close("A prefill scores (third chunk, rows 4096 ... 4199)", to_np(lg_a), refs[0]["logits"][0], atol=LOGIT_TOL)
        assert_close("B prefill scores", to_np(lg_b), refs[1]["logits"][0], atol=LOGIT_TOL)
        for _ in range(PAGED_STEPS - 1):
            eng.seq_decode([a, b])
        torch.cuda.synchronize()
        pa, pb = eng.seq_pages(a), eng.seq_pages(b)
        assert len(pa) == 66 and len(pb) == 1 and not set(pa) & set(pb), (pa, pb)
        assert pa != list(range(pa[0], pa[0] + len(pa))), "the long sequence's pages are contiguous: the table is not exercised"
        for s, ref, S in ((a, refs[0], lens[0]), (b, refs[1], lens[1])):
            eng.check_device_flag(eng.seq_counters(s).tolist())
            got = eng.seq_tokens(s)[:PAGED_STEPS].tolist()
            print(f"sequence of {S}: oracle {ref['ids'][:PAGED_STEPS]} device {got}")
            assert got == ref["ids"][:PAGED_STEPS], f"sequence of {S} tokens differs from its oracle"
            assert eng.seq_pos(s) == S + PAGED_STEPS - 1
            lp = tuple(x.cpu().numpy().copy() for x in eng.logprobs(s))
            worst = check_sequence(ref["logits"], got, lp, PAGED_LOGPROBS, LOGIT_TOL, what=f"sequence of {S}")
            print(f"sequence of {S}: log-probabilities of {PAGED_STEPS} tokens within {worst:.2e} (bound {2 * LOGIT_TOL:.0e})")
        # one more row of A through the prefill path: it attends to the K / V rows the batched decode steps appended
        last = torch.from_numpy(sd["model.embed_tokens.weight"][refs[0]["ids"][PAGED_STEPS - 1]][None]).to(dev)
        lg = eng.seq_prefill(a, last, want_logits=True)
        assert_close(f"A scores at position {lens[0] + PAGED_STEPS - 1}", to_np(lg), refs[0]["logits"][PAGED_STEPS], atol=LOGIT_TOL)
        assert int(eng.seq_tokens(a)[0].item()) == refs[0]["ids"][PAGED_STEPS]
    finally:
        eng.close()
