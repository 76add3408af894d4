"""Mixed-length audio clips in ONE tower pass (the serving plugin's padded batch, vllm_file/mixtral.py:861-886, 1043-1052):
per-batch key lengths in the rel-pos attention operator, then WhaleAudioEncoder.forward for B >= 2 against the numpy oracle of
every clip ALONE at its own length (oracle/encoders.py whale_encoder, pinned to the reference's padded batch by
tests/test_oracle_pin.py::test_live_whale_padded_batch_vs_reference).
Bars: tiny encoder atol 3e-5, released width atol 1e-3 / rtol 1e-4 (BASELINE.json)."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import encoders as oe
from tests.util import assert_close, to_np
from vita_amd.checkpoint import synth_state_dict
from vita_amd.config import AudioConfig, VitaConfig

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


# ---- operator ------------------------------------------------------------------------------------------------------------------
def _attn(qkv, pos, u, v, B, S, nh, dk, klen=None, klens=None, chunk=0, left=-1):
    from vita_amd import ops
    C = nh * dk
    o = torch.full((B * S, C), float("nan"), dtype=torch.float32, device=qkv.device)
    ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], o, B=B, Hq=nh, Hkv=nh, Sq=S, Sk=S, d=dk, ldq=3 * C, hsq=dk, ldk=3 * C, hsk=dk,
                  ldv=3 * C, hsv=dk, ldo=C, bsq=S * 3 * C, bsk=S * 3 * C, bso=S * C, scale=1.0 / math.sqrt(dk), klen=klen,
                  klens=klens, chunk=chunk, left=left, p=pos, ldp=C, hsp=dk, bias_u=u, bias_v=v)
    return o


@pytest.mark.parametrize("chunk,left", [(0, -1), (7, 2)])
def test_attention_per_batch_key_lengths(dev, chunk, left):
    B, S, nh, dk = 3, 150, 4, 64
    C = nh * dk
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn((B * S, 3 * C), generator=g).to(dev)
    pos = torch.randn((S, C), generator=g).to(dev)
    u, v = (0.3 * torch.randn((nh, dk), generator=g)).to(dev), (0.3 * torch.randn((nh, dk), generator=g)).to(dev)
    kl = [71, 150, 37]                                     # all different, none a multiple of 16, the longest in the middle
    klens = torch.tensor(kl, dtype=torch.int32, device=dev)
    got = _attn(qkv, pos, u, v, B, S, nh, dk, klen=max(kl), klens=klens, chunk=chunk, left=left).view(B, S, C)
    assert torch.isfinite(got).all()
    for b in range(B):
        one = _attn(qkv[b * S:(b + 1) * S], pos, u, v, 1, S, nh, dk, klen=kl[b], chunk=chunk, left=left)
        assert_close(f"klens batch {b} (klen {kl[b]}) vs the B = 1 call", to_np(got[b]), to_np(one), atol=3e-5)
    # ... and the padded keys hold no weight: NaN bits behind a clip's length change nothing
    dirty = qkv.clone().view(B, S, 3 * C)
    for b in range(B):
        dirty[b, kl[b]:, C:] = float("nan")
    again = _attn(dirty.view(B * S, 3 * C), pos, u, v, B, S, nh, dk, klen=max(kl), klens=klens, chunk=chunk, left=left).view(B, S, C)
    for b in range(B):
        assert torch.equal(again[b, :kl[b]], got[b, :kl[b]])
    # klens = None is the scalar call: the same launch and arithmetic as a uniform klens, bit for bit, and as B = 1 calls
    plain = _attn(qkv, pos, u, v, B, S, nh, dk, klen=101, chunk=chunk, left=left)
    uniform = _attn(qkv, pos, u, v, B, S, nh, dk, klen=101, klens=torch.full((B,), 101, dtype=torch.int32, device=dev),
                    chunk=chunk, left=left)
    assert torch.equal(plain, uniform)
    for b in range(B):
        one = _attn(qkv[b * S:(b + 1) * S], pos, u, v, 1, S, nh, dk, klen=101, chunk=chunk, left=left)
        assert torch.equal(plain.view(B, S, C)[b], one)


def test_attention_kernels_without_a_per_batch_form_refuse_klens(dev):
    from vita_amd import _lib, ops
    B, S, nh, dk = 2, 40, 2, 64
    C = nh * dk
    qkv = torch.randn((B * S, 3 * C)).to(dev)
    o = torch.empty((B * S, C), device=dev)
    kw = dict(B=B, Hq=nh, Hkv=nh, Sq=S, Sk=S, d=dk, ldq=3 * C, hsq=dk, ldk=3 * C, hsk=dk, ldv=3 * C, hsv=dk, ldo=C, bsq=S * 3 * C,
              bsk=S * 3 * C, bso=S * C, scale=0.125, klen=33, klens=torch.tensor([33, 21], dtype=torch.int32, device=dev))
    with pytest.raises(_lib.VitaHipError, match="rc=-2"):          # plain call: the bf16 x 3 kernel (VH_E_ARG)
        ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], o, **kw)
    with pytest.raises(_lib.VitaHipError, match="rc=-2"):          # causal
        ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], o, causal=True, **kw)
    with pytest.raises(ValueError):
        ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], o, **dict(kw, klens=torch.tensor([33], dtype=torch.int32, device=dev)))


def test_audio_front_and_tail_kernels(dev):
    from vita_amd import ops
    g = torch.Generator().manual_seed(2)
    B, T, F, C = 3, 41, 80, 64
    feats = torch.randn((B, T, F), generator=g).to(dev)
    mean, istd = torch.randn(F, generator=g).to(dev), (torch.rand(F, generator=g) + 0.5).to(dev)
    w, b = (0.2 * torch.randn((C, 9), generator=g)).to(torch.bfloat16).to(dev), torch.randn(C, generator=g).to(dev)
    out, T1, F1 = ops.audio_conv1_batch(feats, mean, istd, w, b)
    for i in range(B):                                             # per clip the single-clip kernel's arithmetic, bit for bit
        one, t1, f1 = ops.audio_conv1(feats[i], mean, istd, w, b)
        assert (t1, f1) == (T1, F1) and torch.equal(out.view(B, T1 * F1, C)[i], one)
    S, gap = 9, 4
    x = torch.randn((B * S, C), generator=g).to(dev)
    kl = [9, 0, 5]
    y = ops.audio_mask_rows(x, torch.tensor(kl, dtype=torch.int32, device=dev), B, gap).view(B, S + gap, C)
    for i in range(B):
        assert torch.equal(y[i, :kl[i]], x.view(B, S, C)[i, :kl[i]]) and not y[i, kl[i]:].any()


# ---- tower ---------------------------------------------------------------------------------------------------------------------
def _check_batch(enc, sd, acfg, clips, lens, atol, rtol=0.0, chunk=0, left=-1, what="whale batch"):
    """forward on the padded batch vs the oracle on every padded clip alone at its own length: masks equal, valid rows close."""
    dev = enc._device
    out = enc(torch.from_numpy(clips).to(dev), torch.tensor(lens).to(dev))
    emb, mask = out["inputs_embeds"], out["attention_mask"]
    assert emb.shape[0] == len(lens) and mask.shape == emb.shape[:2] and mask.dtype == torch.bool
    for b, L in enumerate(lens):
        ref, rmask = oe.whale_encoder(sd, acfg, clips[b], length=L, chunk=chunk, left=left)[:2]
        m = np.asarray(rmask).astype(bool)
        assert to_np(mask[b]).astype(bool).tolist() == m.tolist(), (b, L)
        assert 0 < m.sum() and (b == int(np.argmax(lens)) or m.sum() < m.shape[0])
        assert_close(f"{what}: clip {b} ({L} frames) valid rows vs oracle", to_np(emb[b])[m], np.asarray(ref)[m], atol=atol, rtol=rtol)
    return emb, mask


@pytest.fixture(scope="module")
def tiny_audio(dev):
    from vita_amd.model.encoders import WhaleAudioEncoder
    cfg = VitaConfig.tiny()
    sd = synth_state_dict(cfg, seed=17, parts=("audio",))
    return WhaleAudioEncoder(sd, acfg=cfg.audio, device=dev, llm_dim=cfg.text.hidden_size), sd, cfg


def _padded(lens, seed, dim=80):
    rng = np.random.default_rng(seed)
    clips = np.zeros((len(lens), max(lens), dim), np.float32)
    for b, L in enumerate(lens):
        clips[b, :L] = rng.standard_normal((L, dim)).astype(np.float32)
    return clips


@pytest.mark.parametrize("per_operator", [False, True])
def test_tiny_tower_three_clips_one_pass(tiny_audio, per_operator):
    enc, sd, cfg = tiny_audio
    lens = [97, 123, 61]                                   # all different, the longest in the MIDDLE
    clips = _padded(lens, seed=7, dim=cfg.audio.input_dim)
    enc.per_operator = per_operator
    try:
        emb, mask = _check_batch(enc, sd, cfg.audio, clips, lens, atol=3e-5)
        # permuting the clips gives every clip the same result
        perm = [2, 0, 1]
        out = enc(torch.from_numpy(clips[perm]).to(enc._device), torch.tensor([lens[i] for i in perm]))
        for j, i in enumerate(perm):
            assert torch.equal(out["attention_mask"][j], mask[i])
            m = mask[i]
            assert_close(f"clip {i} at slot {j} vs slot {i}", to_np(out["inputs_embeds"][j][m]), to_np(emb[i][m]), atol=3e-5)
        # B = 1 keeps the single-clip path: forward is encode_one
        one = enc(torch.from_numpy(clips[1:2]).to(enc._device), torch.tensor([lens[1]]))
        e1, m1 = enc.encode_one(torch.from_numpy(clips[1]).to(enc._device), lens[1])
        assert torch.equal(one["inputs_embeds"][0], e1) and torch.equal(one["attention_mask"][0], m1)
    finally:
        enc.per_operator = False


def test_tiny_tower_chunk_mask_in_the_batch(tiny_audio):
    enc, sd, cfg = tiny_audio
    lens = [97, 123, 61]
    clips = _padded(lens, seed=8, dim=cfg.audio.input_dim)
    enc.set_chunk_mask(5, 1)
    try:
        _check_batch(enc, sd, cfg.audio, clips, lens, atol=3e-5, chunk=5, left=1, what="whale batch, chunk mask")
    finally:
        enc.set_chunk_mask(0, -1)


def test_released_width_two_layers_two_clips(dev):
    from vita_amd.model.encoders import WhaleAudioEncoder
    cfg = VitaConfig()
    cfg.audio = AudioConfig(num_hidden_layers=2)
    sd = synth_state_dict(cfg, seed=23, parts=("audio",))
    enc = WhaleAudioEncoder(sd, acfg=cfg.audio, device=dev, llm_dim=4096)
    short = np.load(os.path.join(GOLD, "q1_audio.npz"))["fbank"]          # real fbank of asset/q1.wav: 352 frames
    lens = [998, short.shape[0]]
    clips = np.zeros((2, 998, 80), np.float32)
    clips[0] = 4.0 * np.random.default_rng(9).standard_normal((998, 80)).astype(np.float32)
    clips[1, :lens[1]] = short
    emb, mask = _check_batch(enc, sd, cfg.audio, clips, lens, atol=1e-3, rtol=1e-4, what="whale real batch")
    assert tuple(emb.shape) == (2, 124, 4096) and int(mask[1].sum()) == 44 and bool(mask[0].all())
