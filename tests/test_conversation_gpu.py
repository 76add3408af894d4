"""Requests with several audio clips of DIFFERENT lengths through the serving surface, and two spoken turns through the duplex
server in conversation mode — ids against the ORACLE: every clip alone through oracle/encoders.py whale_encoder at its own
length, its VALID rows spliced (the serving flavour: audio_feature_size(frames) tokens per clip), oracle/mixtral.py greedy.
Extends tests/oracle_e2e.py (one clip, whole padded rows) for this flavour without touching it."""
import asyncio
import json
import os
import time

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import encoders as oe
from oracle import mixtral as om
from tests import tiny_ckpt
from tests.oracle_e2e import _np

pytestmark = pytest.mark.gpu
IMG_ID, AUD_ID = 990, 991      # stand-ins for 51000 / 51001 inside the tiny 1000-entry vocabulary
CMVN = "model.audio_encoder.encoder.global_cmvn."


def _ckpt(d, seed):
    sd = tiny_ckpt.write(d, seed=seed)
    cj = os.path.join(d, "config.json")
    with open(cj) as f:
        j = json.load(f)
    j.update(image_token_index=IMG_ID, audio_token_index=AUD_ID, min_dynamic_patch=1, max_dynamic_patch=12, use_thumbnail=True)
    with open(cj, "w") as f:
        json.dump(j, f)
    return sd


def _clip(frames, seed):
    """CMVN-normalised features, as WhaleFeatureExtractor hands them to multi_modal_data."""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((frames, 80)).astype(np.float32))


def oracle_request(sd, cfg, ids, images, clips, image_processor, n_new, eos=2):
    """One serving request on the oracle.  ids: the prompt with ONE placeholder id per image / clip; clips: normalised features
    (the oracle's CMVN is switched to the identity for them), padded with zeros to the longest, each encoded ALONE at its own
    length.  -> (greedy ids, inputs_embeds [S, H])."""
    from vita_amd.host.image_processing import dynamic_preprocess
    sdn = dict(sd)
    sdn[CMVN + "mean"], sdn[CMVN + "istd"] = np.zeros_like(sd[CMVN + "mean"]), np.ones_like(sd[CMVN + "istd"])
    embed = np.asarray(sd["model.embed_tokens.weight"], np.float32)
    T = max([int(c.shape[0]) for c in clips] or [0])
    parts, ii, ai = [], 0, 0
    for t in ids:
        if t == IMG_ID:
            tiles, _ = dynamic_preprocess(images[ii], min_num=1, max_num=12, image_size=cfg.vision.image_size, use_thumbnail=True)
            pix = image_processor.preprocess(tiles, return_tensors="pt")["pixel_values"]
            parts += list(np.asarray(oe.projector(sd, oe.internvit_tower(sd, cfg.vision, _np(pix))), np.float32))
            ii += 1
        elif t == AUD_ID:
            c = _np(clips[ai])
            padded = np.zeros((T, c.shape[1]), np.float32)
            padded[:c.shape[0]] = c
            z, mask = oe.whale_encoder(sdn, cfg.audio, padded, length=c.shape[0])[:2]
            parts.append(np.asarray(z, np.float32)[np.asarray(mask).astype(bool)])
            ai += 1
        else:
            parts.append(embed[int(t)][None])
    emb = np.concatenate(parts, 0)
    out, _ = om.MixtralOracle(sd, cfg.text).greedy(emb, n_new, eos=eos)
    return out, emb


@pytest.mark.timeout(600)
def test_two_clips_of_different_lengths_and_an_image(tmp_path, dev):
    from vita_amd.config import VitaConfig
    from vita_amd.serving import LLM, AsyncEngineArgs, AsyncLLMEngine, SamplingParams, audio_feature_size, expanded_token_ids
    d = str(tmp_path)
    sd = _ckpt(d, seed=33)
    cfg = VitaConfig.tiny()
    llm = LLM(model=d, max_new_tokens=32)
    rng = np.random.default_rng(4)
    img = Image.fromarray(rng.integers(0, 255, size=(70, 170, 3), dtype=np.uint8))
    clips = [_clip(211, 1), _clip(87, 2)]                                   # the longer one first
    ids = [1, 5, IMG_ID, 6, AUD_ID, 7, 8, AUD_ID, 9]
    req = {"prompt_token_ids": ids, "multi_modal_data": {"image": [img], "audio": clips}}
    sp = SamplingParams(temperature=0.01, max_tokens=10, skip_special_tokens=False)
    out = llm.generate(req, sampling_params=sp)[0]
    got = out.outputs[0].token_ids
    want, emb = oracle_request(sd, cfg, ids, [img], clips, llm.image_processor, 10)
    sent, _ = llm._expand(ids, [img], clips)
    expanded = expanded_token_ids(sent, [211, 87], image_token_index=IMG_ID, audio_token_index=AUD_ID,
                                  tokens_per_tile=(cfg.vision.image_size // cfg.vision.patch_size // 2) ** 2)
    assert out.metrics["prompt_tokens"] == len(expanded) == emb.shape[0]
    assert expanded.count(AUD_ID) == audio_feature_size(211) + audio_feature_size(87)
    assert 1 <= len(got) <= 10 and got == want[:len(got)] and (len(got) == 10 or got[-1] == 2), (got, want)

    engine = AsyncLLMEngine.from_engine_args(AsyncEngineArgs(model=d, dtype="float16", max_num_seqs=2, max_new_tokens=32,
                                                             kv_pool_tokens=2048, device="cuda:0"))
    try:
        async def run():
            last = None
            async for o in engine.generate(req, sampling_params=sp, request_id="two-clips"):
                last = o
            return last
        again = asyncio.run(run())
    finally:
        engine.shutdown()
    assert again.finished and again.outputs[0].token_ids == got, (again.outputs[0].token_ids, got)


def _drain(q, n, timeout):
    out, t0 = [], time.time()
    while len(out) < n and time.time() - t0 < timeout:
        try:
            out.append(q.get(timeout=0.1))
        except Exception:
            pass
    return out


@pytest.mark.timeout(600)
def test_two_spoken_turns_in_conversation_mode(tmp_path, dev):
    from transformers import AutoTokenizer
    from vita_amd.config import VitaConfig
    from vita_amd.duplex import DuplexServer, make_serving_llm, merge_current_and_history
    from vita_amd.host.prompt import tokenizer_image_audio_token
    from vita_amd.serving import SamplingParams
    d = str(tmp_path)
    sd = _ckpt(d, seed=45)          # a checkpoint on which (by the oracle) the first turn in the prompt changes the second answer
    cfg = VitaConfig.tiny()
    tok = AutoTokenizer.from_pretrained(d)
    clips = [_clip(173, 11), _clip(92, 12)]                                 # two turns never have the same length
    turns = [{"prompt": "<audio>", "multi_modal_data": {"audio": [clips[i]]}, "request_id": i} for i in range(2)]
    n_new = 8
    sp = SamplingParams(temperature=0.01, max_tokens=n_new, skip_special_tokens=False)   # the text shows every id
    srv = DuplexServer(make_serving_llm, (d, 64), sampling_params=sp, conversation=True, history_turns=1)
    try:
        srv.wait_ready(timeout=240)
        stats = []
        for r in turns:
            srv.submit(r)
            stats += _drain(srv.stats, 1, timeout=120)
        hist = [dict(h) for h in srv.history]
    finally:
        srv.close()
    assert [s["id"] for s in stats] == [0, 1] and all(s["error"] is None and not s["negative"] for s in stats), stats
    assert [h["prompt"] for h in hist] == ["<audio>", "<audio>"]
    assert [[tuple(c.shape) for c in h["multi_modal_data"]["audio"]] for h in hist] == [[(173, 80)], [(92, 80)]]   # the UNMERGED requests

    def oracle_turn(history, i):
        merged = merge_current_and_history(history, {"prompt": "<audio>", "multi_modal_data": {"audio": [clips[i]]}},
                                           skip_history_vision=True, move_image_token_to_start=True)
        ids = tokenizer_image_audio_token(merged["prompt"], tok, image_token_index=IMG_ID, audio_token_index=AUD_ID)
        assert ids.count(AUD_ID) == len(merged["multi_modal_data"]["audio"]) == len(history) + 1
        want, _ = oracle_request(sd, cfg, ids, [], merged["multi_modal_data"]["audio"], None, n_new)
        return want

    first = oracle_turn([], 0)
    n0 = stats[0]["n_tokens"]
    assert 1 <= n0 <= n_new and (n0 == n_new or first[n0 - 1] == 2)
    assert hist[0]["response"] == tok.decode(first[:n0], skip_special_tokens=False), (hist[0]["response"], first)
    # the second answer is conditioned on the first turn: its clip, its prompt and its response are in the prompt
    second = oracle_turn([hist[0]], 1)
    n1 = stats[1]["n_tokens"]
    assert 1 <= n1 <= n_new and (n1 == n_new or second[n1 - 1] == 2)
    assert hist[1]["response"] == tok.decode(second[:n1], skip_special_tokens=False), (hist[1]["response"], second)
    alone = oracle_turn([], 1)
    print("second turn with / without memory:", second, alone)
    assert second != alone                                                  # ... so an answer without memory would not have passed
