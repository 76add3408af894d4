"""Score-level parity of batched decode iterations (vh_mixtral_seq_decode -> decode_iteration: k_decb_gemv, k_decb_attn, k_decb_lmhead
and the streamed MoE with one row per sequence) with the fp32 oracle of every request alone.

The id-level tests (tests/test_paged_gpu.py) cannot see a batched kernel that is numerically wrong inside the argmax margin.  Here
every sequence asks for logprobs = 20 with neutral penalties (seq_set_logit_rules), which keeps, per generated token, the chosen
token's log-probability and the top-20 ids and log-probabilities of the raw row; tests/seq_scores.py holds them to the oracle's row of
that step within 2 LOGIT_TOL — the bound that "every logit within LOGIT_TOL" implies, derived there.

One schedule for every case: nine prompts join one by one, the iteration grows through the widths 2, 3, 4, 5, 8, 9 (2: batched
attention with per-sequence expert GEMVs; 3: the smallest streamed MoE; 5 / 8 / 9: groups of 4 + 1 / 4 + 4 / 4 + 4 + 1), then the
sequences leave one by one and the last one runs alone (tests/seq_scores.py batched_schedule).  The list handed to seq_decode is
rotated every iteration, so every sequence — the 130-token one with the most splits among them — moves through the lanes and groups."""
import functools

import numpy as np
import pytest
import torch

from oracle import mixtral as om
from tests import q8_ref
from tests.seq_scores import LENS, LOGIT_TOL, batched_schedule, check_sequence, tokens_per_request
from vita_amd.checkpoint import pack_mixtral, synth_state_dict
from vita_amd.config import TextConfig, VitaConfig

pytestmark = pytest.mark.gpu

K = 20
SEED = 11
MARGIN = 1e-4          # smallest top-1 - top-2 margin a greedy pick of the oracle may have (tests/test_long_context_gpu.py MARGIN)


def _text(geom):
    if geom == "tiny":
        return VitaConfig.tiny().text
    # the 4 : 1 head grouping of tests/test_paged_gpu.py's `flash` case
    return TextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2, intermediate_size=1024,
                      num_local_experts=8, vocab_size=2000)


@functools.lru_cache(maxsize=None)
def _case(geom, experts):
    """weights, prompts and every request's oracle run alone (ids and the raw row of every generated token), computed once per
    geometry and expert type and shared by the cases; nothing here is modified afterwards."""
    cfg = VitaConfig.tiny()
    cfg.text = _text(geom)
    sd = synth_state_dict(cfg, seed=SEED, parts=("text",))
    orc = om.MixtralOracle(q8_ref.dequant_state_dict(sd) if experts == "int8" else sd, cfg.text)
    rng = np.random.default_rng(SEED + 7)
    n_tok = tokens_per_request(batched_schedule())
    reqs = []
    for S, n in zip(LENS, n_tok):
        emb = sd["model.embed_tokens.weight"][rng.integers(3, cfg.text.vocab_size, size=S)]
        orc.reset()
        ids, rows = orc.greedy(emb, n)
        top = np.sort(rows, -1)
        reqs.append(dict(emb=emb, ids=ids, rows=rows, margin=float((top[:, -1] - top[:, -2]).min())))
    return cfg, sd, reqs


def _run(dev, geom, experts, moe_min, want_logprobs):
    """the schedule on one engine -> the requests and, per request, (ids, x): x = the sequence's logprob buffers copied to the host
    (want_logprobs), or whether they are still what they were when the slot was allocated (logprobs never requested)."""
    from vita_amd import _lib
    from vita_amd.engine import MixtralEngine
    cfg, sd, reqs = _case(geom, experts)
    steps = batched_schedule()
    n_tok = tokens_per_request(steps)
    eng = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev, experts=experts), dev, max_ctx=2048, max_prefill=max(LENS) + 8,
                        max_new=max(n_tok) + 4, max_seqs=9, max_logprobs=K)
    slot, out, fresh = {}, {}, {}
    _lib.tune("batch_moe_min", moe_min)
    try:
        for kind, arg in steps:
            if kind == "join":
                s = slot[arg] = eng.seq_alloc()
                if want_logprobs:
                    eng.seq_set_logit_rules(s, logprobs=K)
                else:
                    torch.cuda.synchronize()
                    fresh[arg] = [t.clone() for t in eng.logprobs(s)]
                eng.seq_prefill(s, torch.from_numpy(reqs[arg]["emb"]).to(dev))
            elif kind == "decode":
                eng.seq_decode([slot[i] for i in arg])
            else:
                s = slot.pop(arg)
                torch.cuda.synchronize()
                eng.check_device_flag(eng.seq_counters(s).tolist())
                assert eng.seq_pos(s) == LENS[arg] + n_tok[arg] - 1
                ids = eng.seq_tokens(s)[:n_tok[arg]].tolist()
                lp = eng.logprobs(s)
                if want_logprobs:
                    out[arg] = (ids, tuple(t.cpu().numpy().copy() for t in lp))
                else:
                    out[arg] = (ids, all(torch.equal(a, b) for a, b in zip(lp, fresh[arg])))
                eng.seq_free(s)
    finally:
        _lib.tune("batch_moe_min", 3)
        eng.close()
    return reqs, out


@pytest.mark.parametrize("geom,experts,moe_min", [("tiny", "bf16", 3), ("tiny", "bf16", 0), ("heads-8-2", "bf16", 3),
                                                  ("heads-8-2", "bf16", 0), ("tiny", "int8", 3), ("tiny", "int8", 0)])
def test_batched_iterations_match_the_oracle_scores(dev, geom, experts, moe_min):
    """every generated token of every sequence (entry 0, the prefill's head, included): the id is the oracle's, and the token's
    log-probability and the top-20 list pass check_step against the oracle's row of that step.  int8 experts: the oracle runs on the
    dequantised weights the engine computes with."""
    reqs, out = _run(dev, geom, experts, moe_min, True)
    worst = 0.0
    for i, r in enumerate(reqs):
        # an id that differs is a wrong kernel and never a tie (the bar of tests/test_long_context_gpu.py: the errors are ~1e-5)
        assert r["margin"] > MARGIN, f"request {i}: a greedy pick of the oracle is a tie ({r['margin']:.2e}): choose another seed"
        ids, lp = out[i]
        assert ids == r["ids"], f"request {i} (prompt {LENS[i]}): device {ids} vs oracle {r['ids']}"
        worst = max(worst, check_sequence(r["rows"], ids, lp, K, LOGIT_TOL, what=f"request {i} (prompt {LENS[i]})"))
    print(f"{geom} {experts} batch_moe_min = {moe_min}: {sum(len(r['ids']) for r in reqs)} tokens, "
          f"worst log-probability error {worst:.2e} (bound {2 * LOGIT_TOL:.0e})")


def test_ids_do_not_depend_on_kept_scores(dev):
    """off is off: the same schedule with logprobs never requested gives the same ids, and the sequences' logprob buffers stay as
    they were when the slot was allocated — keeping the rows is not what makes the batched path right."""
    reqs, out = _run(dev, "tiny", "bf16", 3, False)
    for i, r in enumerate(reqs):
        ids, untouched = out[i]
        assert ids == r["ids"], f"request {i} (prompt {LENS[i]}): device {ids} vs oracle {r['ids']}"
        assert untouched, f"request {i}: logprob buffers were written although logprobs were never requested"
