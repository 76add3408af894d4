"""Inputs the MXFP4 engine tests share: the GPU tests (tests/test_experts_mxfp4_gpu.py) compare ids with == and logits
within LOGIT_TOL against the fp32 oracle on w', which is only a well-posed bar when the oracle's top-2 logit gap is at least
2 * LOGIT_TOL at every generated step; tests/test_experts_mxfp4_cpu.py checks that precondition for every case listed here."""
import numpy as np

from oracle import mixtral as om
from tests import q4_ref
from vita_amd.checkpoint import synth_state_dict
from vita_amd.config import VitaConfig  # noqa: F401  (re-exported for the tests)

LOGIT_TOL = 1e-3
ENGINE_SEED, ENGINE_S, ENGINE_NEW = 4, 37, 17          # one request: prompt rng default_rng(ENGINE_SEED + 100)
SEQ_SEED, SEQ_N, SEQ_NEW = 4, 6, 6                     # six sequences: prompts of 5 + 3 i rows from default_rng(7)
SEQ_BATCH = (1, 4)                                     # the two of them that also go through seq_prefill_batch
CKPT_SEED = 23                                         # tests/tiny_ckpt.py checkpoint of the public-surface tests
CKPT_LOAD_IDS, CKPT_LOAD_NEW = [1, 5, 6, 7, 8, 9, 10, 11, 12], 6
CKPT_LLM_IDS, CKPT_LLM_NEW = [1, 5, 6, 7, 8], 4


def tiny_text_sd(seed):
    cfg = VitaConfig.tiny()
    return cfg, synth_state_dict(cfg, seed=seed, parts=("text",))


def engine_prompt(sd, cfg):
    rng = np.random.default_rng(ENGINE_SEED + 100)
    return sd["model.embed_tokens.weight"][rng.integers(3, cfg.text.vocab_size, size=ENGINE_S)]


def seq_prompts(sd, cfg):
    rng = np.random.default_rng(7)
    return [sd["model.embed_tokens.weight"][rng.integers(3, cfg.text.vocab_size, size=5 + 3 * i)] for i in range(SEQ_N)]


def oracle_on_wprime(sd, cfg):
    return om.MixtralOracle(q4_ref.dequant_state_dict(sd), cfg.text)


def greedy(orc, emb, n):
    """(ids, logits [n][V], smallest top-2 gap over the n steps) of the oracle on one prompt"""
    orc.reset()
    ids, lg = orc.greedy(emb, n)
    top = np.sort(np.asarray(lg, np.float64), -1)
    return ids, lg, float((top[:, -1] - top[:, -2]).min())
