"""vLLM-shaped serving surface (SURVEY §8(b) flavour 2 / §8(f)#1) over the HIP engine.

What the reference's web demo does with vLLM (web_demo/web_ability_demo.py:132-243,340-351):

    llm = LLM(model=path, dtype="float16", tensor_parallel_size=2, limit_mm_per_prompt={...})
    sampling_params = SamplingParams(temperature=0.01, max_tokens=512, best_of=1, skip_special_tokens=False)
    out = llm.generate({"prompt_token_ids": ids, "multi_modal_data": {"image": [PIL...], "audio": [Tensor[T,80]...]}},
                       sampling_params=sampling_params)
    text = out[0].outputs[0].text

keeps working with `from vita_amd.serving import LLM, SamplingParams`.  The prompt carries ONE
`image_token_index` (51000) per image and ONE `audio_token_index` (51001) per clip; like the plugin's
input processor (web_demo/vllm_tools/vllm_file/mixtral.py:194-311) we tile each image with
dynamic_preprocess (+thumbnail), expand its placeholder to 256 tokens per tile and each audio placeholder to
`((T-1)//2-1)//2 -> (.-1)//2+1` tokens.  Audio features arrive CMVN-normalised by WhaleFeatureExtractor (the
vLLM audio tower has no global_cmvn: mixtral.py:1245-1247), so the encoder is run with `normalized=True`.
Sampling: a request with SamplingParams(seed=...) and temperature > 0 is sampled on the device (temperature -> top_k -> top_p,
Gumbel-max over a Philox stream keyed by the seed: include/vita_hip.h vh_sampling), so its ids are a function of the request;
unseeded temperature <= 0.01 is greedy (the demo's setting) and unseeded sampling above it raises.

Concurrent requests (the interactive demo's AsyncLLMEngine, web_interactive_demo.py:126,315-328,942-951): the engine's
KV cache is a pool of 64-token pages addressed through per-sequence block tables (vh_mixtral_seq_* in
include/vita_hip.h); `ContinuousBatcher` is the iteration-level scheduler over it (admit -> prefill, one decode step for
every running sequence per iteration, free on finish, preempt-by-recompute when the pool runs dry) and
`AsyncLLMEngine.generate(inputs, sampling_params, request_id)` is the async iterator the demo consumes.  `LLM.generate`
(the offline demo) keeps serving one request at a time on the same engine."""
import asyncio
import collections
import hashlib
import json
import os
import threading
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from .host.constants import AUDIO_TOKEN_INDEX, IMAGE_TOKEN_INDEX
from .host.image_processing import dynamic_preprocess


@dataclass
class SamplingParams:
    temperature: float = 0.01
    max_tokens: int = 512
    best_of: int = 1
    skip_special_tokens: bool = False
    stop_token_ids: Optional[List[int]] = None
    top_p: float = 1.0
    top_k: int = -1
    seed: Optional[int] = None
    # logit rules on the device (include/vita_hip.h vh_logit_rules), vLLM's names and ranges: the penalties see the request's
    # expanded prompt ids and its output so far; logprobs = K returns, per generated token, the top K and the chosen id under
    # log_softmax of the RAW logits (vLLM's default)
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logprobs: Optional[int] = None

    def __post_init__(self):
        if not 0.0 < float(self.repetition_penalty) <= 2.0:
            raise ValueError(f"repetition_penalty must be in (0, 2], got {self.repetition_penalty}")
        for name in ("presence_penalty", "frequency_penalty"):
            if not -2.0 <= float(getattr(self, name)) <= 2.0:
                raise ValueError(f"{name} must be in [-2, 2], got {getattr(self, name)}")
        if self.logprobs is not None and not 0 <= int(self.logprobs) <= 20:
            raise ValueError(f"logprobs must be in [0, 20], got {self.logprobs}")


def rules_of(sp):
    """the logit rules of a request (keywords of MixtralEngine.set_logit_rules / seq_set_logit_rules without the ids), or None when
    it has neither penalties nor logprobs."""
    if sp is None:
        return None
    r, p, f = float(sp.repetition_penalty), float(sp.presence_penalty), float(sp.frequency_penalty)
    if r == 1.0 and p == 0.0 and f == 0.0 and sp.logprobs is None:
        return None
    return dict(repetition_penalty=r, presence_penalty=p, frequency_penalty=f, logprobs=-1 if sp.logprobs is None else int(sp.logprobs))


def sampling_of(sp):
    """the device sampling of a request (dict for MixtralEngine.set_sampling / seq_set_sampling), or None for greedy: seeded
    requests with temperature > 0 sample; vLLM's top_k = -1 (off) is 0."""
    if sp is None or sp.seed is None or not sp.temperature or sp.temperature <= 0:
        return None
    top_k = 0 if sp.top_k is None or int(sp.top_k) < 0 else int(sp.top_k)
    return dict(temperature=float(sp.temperature), top_k=top_k, top_p=1.0 if sp.top_p is None else float(sp.top_p), seed=int(sp.seed))


def sample_kwargs(sp):
    """generate() keywords of a request"""
    s = sampling_of(sp)
    return dict(do_sample=False) if s is None else dict(do_sample=True, **s)


@dataclass
class CompletionOutput:
    index: int
    text: str
    token_ids: List[int]
    finish_reason: str = "length"
    logprobs: Optional[List[dict]] = None           # SamplingParams(logprobs=K): per token {id: logprob}, the top K + the chosen id
    cumulative_logprob: Optional[float] = None      # sum of the chosen ids' log-probabilities


@dataclass
class RequestOutput:
    request_id: str
    prompt_token_ids: List[int]
    outputs: List[CompletionOutput] = field(default_factory=list)
    finished: bool = True
    metrics: dict = field(default_factory=dict)
    num_cached_tokens: int = 0                      # prompt tokens whose K/V came from the prefix cache (vLLM's name; 0 without it)


def audio_feature_size(n_frames: int) -> int:
    """mixtral.py:283-287."""
    down = ((int(n_frames) - 1) // 2 - 1) // 2
    return (down - 1) // 2 + 1


def expand_placeholders(ids, images, audios, *, image_token_index, audio_token_index, image_size, min_dynamic_patch=1,
                        max_dynamic_patch=12, use_thumbnail=True, limit_mm=None):
    """The plugin's input processor (web_demo/vllm_tools/vllm_file/mixtral.py:194-295) in the HF-flavour vocabulary:
    every image placeholder becomes one IMAGE sentinel per TILE of dynamic_preprocess (+ thumbnail), every audio
    placeholder one AUDIO sentinel; the splice later widens a sentinel to 256 tokens per tile / audio_feature_size
    tokens per clip, which is the reference's repeat_and_pad_image_tokens (:100-190) with repeat counts
    256 * tiles and ((T-1)//2-1)//2 -> (.-1)//2+1 (:283-287).  Returns (sentinel ids, tiles)."""
    limit_mm = limit_mm or {}
    n_img, n_aud = ids.count(image_token_index), ids.count(audio_token_index)
    if n_img != len(images) or n_aud != len(audios):
        raise ValueError(f"prompt has {n_img} image / {n_aud} audio placeholders but multi_modal_data holds "
                         f"{len(images)} / {len(audios)}")                    # mixtral.py:136-140,1110-1124
    if len(images) > limit_mm.get("image", 256) or len(audios) > limit_mm.get("audio", 50):
        raise ValueError("limit_mm_per_prompt exceeded")
    tiles, out, ii = [], [], 0
    for t in ids:
        if t == image_token_index:
            ts, _ = dynamic_preprocess(images[ii], min_num=min_dynamic_patch, max_num=max_dynamic_patch,
                                       image_size=image_size, use_thumbnail=use_thumbnail)
            tiles += ts
            out += [IMAGE_TOKEN_INDEX] * len(ts)
            ii += 1
        elif t == audio_token_index:
            out.append(AUDIO_TOKEN_INDEX)
        else:
            out.append(int(t))
    return out, tiles


def expanded_token_ids(sentinel_ids, audio_frames, *, image_token_index, audio_token_index, tokens_per_tile=256):
    """The id sequence the reference's input processor hands to vLLM (`new_token_ids`, mixtral.py:175-190,289-295),
    rebuilt from the sentinel form: what the spliced embedding sequence corresponds to, position by position."""
    out, ai = [], 0
    for t in sentinel_ids:
        if t == IMAGE_TOKEN_INDEX:
            out += [image_token_index] * tokens_per_tile
        elif t == AUDIO_TOKEN_INDEX:
            out += [audio_token_index] * audio_feature_size(audio_frames[ai])
            ai += 1
        else:
            out.append(int(t))
    return out


def completion(index, text, token_ids, reason, logprobs=None):
    """CompletionOutput with .logprobs / .cumulative_logprob filled from the per-token {id: logprob} dicts (None: not asked for)."""
    out = CompletionOutput(index, text, token_ids, reason)
    if logprobs is not None:
        out.logprobs = logprobs[:len(token_ids)]
        out.cumulative_logprob = float(sum(d[t] for d, t in zip(out.logprobs, token_ids)))
    return out


class LLM:
    def __init__(self, model, dtype=None, tensor_parallel_size=1, trust_remote_code=True, gpu_memory_utilization=None,
                 disable_custom_all_reduce=True, limit_mm_per_prompt=None, max_new_tokens=1024, device="cuda",
                 max_num_seqs=0, kv_pool_tokens=None, quantization=None, max_logprobs=0, penalty_tables=None,
                 enable_prefix_caching=False, **_):
        from .model.builder import load_pretrained_model
        # vLLM's switch: AsyncLLMEngine's batcher then keeps finished prompts' KV pages under content keys (PrefixCache).  generate()
        # here serves one request at a time on the contiguous pool and does not use the cache; the engine refuses it while the cache
        # holds pages (its error names reset_prefix_cache)
        self.enable_prefix_caching = bool(enable_prefix_caching)
        # vLLM's quantization="experts_int8": the MoE experts as int8 with per-output-row scales
        if quantization not in (None, "experts_int8"):
            raise ValueError(f"quantization={quantization!r}: vita_amd supports None and 'experts_int8'")
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if tensor_parallel_size != 1 and tensor_parallel_size != world:
            raise RuntimeError(
                f"tensor_parallel_size={tensor_parallel_size}: vita_amd runs one process per GPU — launch this program "
                f"with `python -m torch.distributed.run --nproc-per-node {tensor_parallel_size} ...` (WORLD_SIZE={world})")
        self.limit_mm = dict(limit_mm_per_prompt or {"image": 256, "audio": 50})
        kw = {}
        if world > 1:
            kw.update(rank=int(os.environ.get("RANK", "0")), world=world)
            device = f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}"
        if world > 1:
            torch.cuda.set_device(torch.device(device))       # kernels launch on the CURRENT device's stream
        self.tokenizer, self.model, self.image_processor, _ = load_pretrained_model(
            model, None, os.path.basename(str(model).rstrip("/")), "mixtral-8x7b", device=device,
            max_new_tokens=max_new_tokens, max_seqs=int(max_num_seqs), kv_pool_tokens=kv_pool_tokens,
            gpu_memory_utilization=gpu_memory_utilization, load_8bit=quantization == "experts_int8",
            # max_logprobs > 0 (vLLM's name): logprob buffers AND token tables for the engine and every sequence slot, so that
            # SamplingParams' penalties and logprobs run on the device; penalty_tables=True alone: the tables only
            max_logprobs=int(max_logprobs), penalty_tables=bool(max_logprobs) if penalty_tables is None else bool(penalty_tables), **kw)
        self.collective = "none"
        if world > 1:
            from .parallel import setup_tensor_parallel
            self.collective = setup_tensor_parallel(self.model.engine, kw["rank"], world, device,
                                                    backend=os.environ.get("VITA_AMD_DIST_BACKEND", "nccl"))
        with open(os.path.join(model, "config.json")) as f:
            j = json.load(f)
        self.image_token_index = int(j.get("image_token_index", 51000))
        self.audio_token_index = int(j.get("audio_token_index", 51001))
        self.min_dynamic_patch = int(j.get("min_dynamic_patch", 1))
        self.max_dynamic_patch = int(j.get("max_dynamic_patch", 12))
        self.use_thumbnail = bool(j.get("use_thumbnail", True))
        self._n = 0

    def get_tokenizer(self):
        return self.tokenizer

    # ---- one request ----------------------------------------------------------------------------
    def _expand(self, ids, images, audios):
        return expand_placeholders(ids, images, audios, image_token_index=self.image_token_index,
                                   audio_token_index=self.audio_token_index,
                                   image_size=self.image_processor.crop_size["height"],
                                   min_dynamic_patch=self.min_dynamic_patch, max_dynamic_patch=self.max_dynamic_patch,
                                   use_thumbnail=self.use_thumbnail, limit_mm=self.limit_mm)

    @torch.no_grad()
    def _prepare(self, inp, sp: SamplingParams):
        """host side of one request: ids, placeholder expansion, pixel / fbank tensors (what vLLM's input processor and
        mapper do: mixtral.py:194-311).  Returns dict(ids, sent, pix, feats, lens, normalized, max_tokens, eos)."""
        if isinstance(inp, str):
            inp = {"prompt": inp}
        ids = inp.get("prompt_token_ids")
        if ids is None:
            ids = list(self.tokenizer(inp["prompt"]).input_ids)
        ids = [int(x) for x in (ids.tolist() if hasattr(ids, "tolist") else ids)]
        mm = inp.get("multi_modal_data") or {}
        images = mm.get("image", [])
        images = images if isinstance(images, list) else [images]
        audios = mm.get("audio", [])
        audios = audios if isinstance(audios, list) else [audios]
        if sampling_of(sp) is None and sp.temperature is not None and sp.temperature > 0.011:
            raise NotImplementedError("vita_amd samples only with a seed: pass SamplingParams(seed=...) "
                                      "(unseeded temperature <= 0.01 stays greedy, the reference demo's setting)")
        dev = self.model.device
        max_tokens = min(int(sp.max_tokens), int(self.model.max_new_tokens))   # the engine's output buffer is the hard cap
        sent, tiles = self._expand(ids, images, audios)
        size = self.image_processor.crop_size["height"]
        if tiles:
            pix = self.image_processor.preprocess(tiles, return_tensors="pt")["pixel_values"].to(dev)
        else:
            pix = torch.zeros((1, 3, size, size), device=dev)                  # the demo's dummy image
        enc = self.model.get_audio_encoder()
        normalized = False
        if audios:
            if len(audios) > 1:
                T = max(int(a.shape[0]) for a in audios)
                feats = torch.zeros((len(audios), T, audios[0].shape[1]))
                for i, a in enumerate(audios):
                    feats[i, :a.shape[0]] = a.float()
            else:
                feats = audios[0].float()[None]
            lens = torch.tensor([int(a.shape[0]) for a in audios])
            normalized = True                # WhaleFeatureExtractor already applied CMVN
        else:
            feats, lens = torch.zeros((1, 400, enc.acfg.input_dim)), torch.tensor([400])
        eos = {self.model.generation_config.eos_token_id, *(sp.stop_token_ids or [])} - {None}
        rules, prompt_set = rules_of(sp), None
        if rules is not None:
            eng = self.model.engine
            pen = (rules["repetition_penalty"], rules["presence_penalty"], rules["frequency_penalty"]) != (1.0, 0.0, 0.0)
            if (pen and not eng.c.penalty_tables) or rules["logprobs"] > eng.c.max_logprobs:
                raise ValueError(f"penalties / logprobs={sp.logprobs} need LLM(max_logprobs=K) with K >= logprobs "
                                 f"(this engine: max_logprobs={eng.c.max_logprobs}, penalty_tables={bool(eng.c.penalty_tables)})")
            # the prompt set of the penalties: the ids vLLM sees as prompt_token_ids (placeholders widened); ids that are not rows
            # of the LM head can never be generated and are left out
            frames = [int(a.shape[0]) for a in audios]
            exp = expanded_token_ids(sent, frames, image_token_index=self.image_token_index, audio_token_index=self.audio_token_index)
            V = int(self.model.config.vocab_size)
            prompt_set = sorted({t for t in exp if 0 <= t < V})
        return dict(ids=ids, sent=sent, pix=pix, feats=feats.to(dev), lens=lens.to(dev), normalized=normalized,
                    max_tokens=max_tokens, eos=eos, rules=rules, prompt_set=prompt_set)

    @torch.no_grad()
    def _embed(self, req):
        """encoders + splice of a prepared request -> inputs_embeds [S, H] fp32 on the device."""
        enc = self.model.get_audio_encoder()
        enc.normalized_input = req["normalized"]
        try:
            dev = self.model.device
            out = self.model.prepare_inputs_labels_for_multimodal(
                torch.tensor([req["sent"]], dtype=torch.long, device=dev), None, None, None, None, req["pix"],
                {"audios": req["feats"], "lengths": req["lens"]}, audio_valid_rows=True)
        finally:
            enc.normalized_input = False
        return out[4][0].to(torch.float32)

    @torch.no_grad()
    def _one(self, inp, sp: SamplingParams, streamer=None):
        req = self._prepare(inp, sp)
        ids, sent, pix, feats, lens, max_tokens = (req[k] for k in ("ids", "sent", "pix", "feats", "lens", "max_tokens"))
        dev = self.model.device
        enc = self.model.get_audio_encoder()
        enc.normalized_input = req["normalized"]
        rules = req.get("rules")
        rkw = {} if rules is None else dict(repetition_penalty=rules["repetition_penalty"], presence_penalty=rules["presence_penalty"],
                                             frequency_penalty=rules["frequency_penalty"], penalty_prompt_ids=req["prompt_set"],
                                             output_logprobs=rules["logprobs"] if rules["logprobs"] >= 0 else None)
        try:
            out = self.model.generate(torch.tensor([sent], dtype=torch.long, device=dev), images=pix,
                                      audios={"audios": feats.to(dev), "lengths": lens.to(dev)}, num_beams=1,
                                      return_dict_in_generate=True, max_new_tokens=max_tokens,
                                      eos_token_id=list(req["eos"]), streamer=streamer, audio_valid_rows=True,
                                      **sample_kwargs(sp), **rkw)
        finally:
            enc.normalized_input = False
        gen = out.sequences[0, len(sent):].tolist()
        eos = req["eos"]
        reason = "stop" if gen and gen[-1] in eos else "length"
        text = self.tokenizer.decode(gen, skip_special_tokens=sp.skip_special_tokens)
        self._n += 1
        lps = getattr(out, "logprobs", None)
        return RequestOutput(request_id=str(self._n - 1), prompt_token_ids=ids,
                             outputs=[completion(0, text, gen, reason, lps)], metrics=dict(self.model.last_timing))

    def generate_stream(self, inputs, sampling_params: SamplingParams = None, request_id=None, should_stop=None):
        """Generator of RequestOutput with the CUMULATIVE text after every decode window — the shape of
        AsyncLLMEngine.generate's async iterator as web_interactive_demo.py:315-328 consumes it.  `should_stop()`
        is polled between windows; returning True interrupts the request (the duplex monitor hand-off)."""
        import queue
        import threading
        sp = sampling_params or SamplingParams()
        q = queue.Queue()
        state = {"toks": [], "abandoned": False}

        def streamer(new):
            state["toks"] += list(new)
            q.put(list(state["toks"]))
            # abandoned: the consumer left the iterator (noise verdict, interrupt): stop at the next window instead of
            # decoding to EOS / max_tokens while the worker waits in th.join() (the reference aborts the request)
            return not (state["abandoned"] or (should_stop is not None and should_stop()))

        result = {}

        def run():
            try:
                result["out"] = self._one(inputs, sp, streamer=streamer)
            except BaseException as e:  # surfaced to the consumer
                result["err"] = e
            q.put(None)

        old_la = self.model.lookahead
        self.model.lookahead = 2                       # short windows: the interrupt is seen within 2 tokens
        th = threading.Thread(target=run, daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                yield RequestOutput(request_id=str(request_id), prompt_token_ids=[], finished=False,
                                    outputs=[CompletionOutput(0, self.tokenizer.decode(
                                        item, skip_special_tokens=sp.skip_special_tokens), item, "")])
        finally:
            state["abandoned"] = True
            th.join()
            self.model.lookahead = old_la
        if "err" in result:
            raise result["err"]
        yield result["out"]

    def generate(self, prompts, sampling_params: SamplingParams = None, use_tqdm=False, **_):
        sp = sampling_params or SamplingParams()
        batch = prompts if isinstance(prompts, list) else [prompts]
        return [self._one(p, sp) for p in batch]


# ---- prefix caching: KV pages of earlier prompts, found again by content -----------------------------------------------------
PREFIX_ROOT_KEY = hashlib.blake2b(b"vita_amd prefix cache v1", digest_size=16).digest()      # key_{-1} of every chain


def chain_keys(digests, cols, parent=PREFIX_ROOT_KEY):
    """digests: the 16-byte content digests of consecutive 64-row blocks (vh_hash_row_blocks) -> their chain keys
    key_b = blake2b(key_{b-1} || digest_b || cols as 8 little-endian bytes, digest_size=16): a key names the WHOLE prefix up to and
    including its block, for rows of that width."""
    keys, tail = [], int(cols).to_bytes(8, "little")
    for d in digests:
        parent = hashlib.blake2b(parent + bytes(d) + tail, digest_size=16).digest()
        keys.append(parent)
    return keys


def device_digests(rows):
    """fp32 [n, H] device rows -> the digests of its complete 64-row blocks as 16-byte strings: ONE vh_hash_row_blocks launch and one
    small device-to-host copy, which waits for the stream — the only synchronisation prefix caching adds."""
    from . import ops
    if int(rows.shape[0]) < 64:
        return []
    words = ops.hash_row_blocks(rows).cpu().numpy()
    return [words[b].tobytes() for b in range(words.shape[0])]


class PrefixCache:
    """Store of the prefix cache (vLLM's enable_prefix_caching over this engine's pages): chain key -> [page, parent key, children,
    last-use tick].  Every entry owns ONE hold of its page (MixtralEngine.seq_hold_prefix), so the page outlives the sequence that
    wrote it; a sequence that adopts it (seq_adopt) adds its own count.  The entries form a forest closed under `parent`: a block is
    cached only together with the whole prefix in front of it.

    Nothing here looks at a clock or iterates a dict of unequal things in hash order: `tick` is a counter the batcher bumps per
    admitted request, eviction orders by (tick, key).  Tensor-parallel ranks fed the same requests reach the same decisions.

    Eviction: only entries whose page has page_refs == 1 (the cache's hold alone), unpinned and without children; least recently
    used first; exactly as many as asked for.

    The device digest is a content hash, not a cryptographic one (include/vita_hip.h vh_hash_row_blocks): a miss is always safe, a
    false hit would not be, which is why the cache is opt-in."""

    def __init__(self, engine, digests=None):
        self.eng = engine
        self.digests = digests or device_digests
        self.entries = {}
        self.pinned = set()               # pages a request of the current admission pass is about to adopt
        self.tick = 0
        self.evictions = 0

    def keys_after(self, keys, rows):
        """keys of the complete blocks of `rows`, which continue the prefix whose keys are `keys`."""
        return chain_keys(self.digests(rows), int(rows.shape[1]), keys[-1] if keys else PREFIX_ROOT_KEY)

    def match(self, keys, limit):
        """-> pages of the longest cached chain among the first `limit` keys; the chain is touched."""
        pages = []
        for k in keys[:max(int(limit), 0)]:
            e = self.entries.get(k)
            if e is None:
                break
            e[3] = self.tick
            pages.append(e[0])
        return pages

    def insert(self, key, parent, page):
        """`page` (already held once for the cache) under `key`; parent: the key in front of it, None for block 0."""
        self.entries[key] = [int(page), parent, 0, self.tick]
        if parent is not None:
            self.entries[parent][2] += 1

    def _idle(self, e):
        return e[0] not in self.pinned and self.eng.page_refs(e[0]) == 1

    def evictable(self):
        """entries evict() could remove: idle ones all of whose descendants are idle."""
        blocked = set()
        for k, e in self.entries.items():
            if not self._idle(e):
                while k is not None and k not in blocked:
                    blocked.add(k)
                    k = self.entries[k][1]
        return len(self.entries) - len(blocked)

    def evict(self, n):
        """give up to n pages back to the pool -> how many."""
        done = 0
        while done < n:
            # the least recently used childless idle entry, ties by key; a chain shares one tick and only its leaf is childless: the
            # parent becomes a candidate when the leaf is gone
            leaves = sorted((e[3], k) for k, e in self.entries.items() if e[2] == 0)
            k = next((k for _, k in leaves if self._idle(self.entries[k])), None)
            if k is None:
                break
            page, parent = self.entries.pop(k)[:2]
            if parent is not None:
                self.entries[parent][2] -= 1
            self.eng.pages_release([page])
            done += 1
        self.evictions += done
        return done

    def clear(self):
        """drop every entry and its hold (pages a running sequence adopted stay that sequence's until it ends)."""
        pages = sorted(e[0] for e in self.entries.values())
        self.entries.clear()
        self.pinned.clear()
        if pages:
            self.eng.pages_release(pages)


# ---- concurrent requests: iteration-level scheduling over the paged KV cache -------------------------------------------
class ContinuousBatcher:
    """The scheduler half of vLLM's engine for this path (what drives the plugin's forward with `kv_caches` +
    `attn_metadata`, vllm_file/mixtral.py:1130-1186), over `MixtralEngine.seq_*`:

      add(request_id, embeds, max_tokens, eos)   queue a request (FIFO)
      step() -> [(request_id, new_token_ids, finished, finish_reason)]   one iteration:
          1. admit waiting requests while a sequence slot is free and the pool holds the prompt's pages plus one page of
             headroom per running sequence; the admitted prompts are then prefilled in groups of up to max_prefill rows, a
             group of two or more in ONE pass over the weights (seq_prefill_batch: vLLM's max_num_batched_tokens), a
             group of one — or a re-prompt longer than max_prefill, in chunks — by seq_prefill;
          2. if the running sequences need more new pages than the pool has, preempt the youngest ones (free their pages,
             re-queue them at the front with prompt + generated tokens as the new prompt: vLLM's recompute preemption);
          3. `window` greedy decode steps for every running sequence (one C call per step), ONE host synchronisation,
             then eos / max_tokens per sequence; finished sequences return their pages.
      abort(request_id)

    A sequence's ids do not depend on what else is scheduled (same kernels, same arithmetic per sequence); tokens decoded
    past an eos inside a window are discarded, as MixtralEngine's single-request lookahead does.

    prefix_cache=True (or a PrefixCache): vLLM's enable_prefix_caching.  On admission the prompt's 64-row blocks are keyed by content
    (one vh_hash_row_blocks launch + one small device-to-host copy per admitted request: the only synchronisation the feature adds);
    the longest cached chain, at most (S - 1) // 64 pages since one row must be prefilled for the first token's logits, is adopted
    (seq_alloc, seq_adopt) and only emb[64 * hit:] is prefilled, as a member of the admission group like any other prompt (it counts
    S - 64 * hit rows against max_prefill).  Right after a request's prefill is enqueued its full prompt pages that are not cached yet
    are held and inserted — everything runs on one stream, so an adopter's kernels are ordered after the writer's; two requests of
    the SAME admission group therefore do not share.  With an embed_tokens hook, a request that finishes, is aborted or is preempted
    also registers its pages that lie entirely below its position, the ones filled by generated tokens included (keys continue the
    chain over cat(open block's prompt rows, embed_tokens(out[:-1]))): a follow-up turn that repeats prompt + response finds them,
    and a preempted request finds its own pages.  Pool accounting is "free + evictable - promised"; cached pages are evicted
    (childless first, least recently used first, exactly as many as needed) before any running sequence is preempted.
    stats: prefix_queries (lookups), prefix_hit_tokens, prefix_evictions, prefill_rows (rows sent to prefill calls, counted with the
    cache off as well); cached_tokens[request id] is the hit of a request's first admission (the caller pops it)."""

    def __init__(self, engine, embed_tokens=None, max_batch=None, window=1, prefix_cache=False):
        self.eng, self.embed_tokens = engine, embed_tokens
        self.cache = prefix_cache if isinstance(prefix_cache, PrefixCache) else (PrefixCache(engine) if prefix_cache else None)
        self.cached_tokens = {}
        self.max_batch = int(max_batch or engine.c.max_seqs)
        if engine.c.max_seqs < 1:
            raise ValueError("the engine was created without sequence slots (max_seqs = 0)")
        self.window = int(window)
        self.waiting = collections.deque()
        self.running = []                 # admission order
        self.errors = {}                  # request id -> exception of a request that failed alone (event reason "error")
        self.stats = {"iterations": 0, "prefills": 0, "prefill_calls": 0, "preemptions": 0, "decode_steps": 0, "failed": 0,
                      "prefix_queries": 0, "prefix_hit_tokens": 0, "prefix_evictions": 0, "prefill_rows": 0}
        self.logprobs = {}                # request id -> per-token {id: logprob} of requests with rules["logprobs"] >= 0; the entry of a
                                          # finished request stays until the caller pops it (a failed or aborted one is dropped here)

    def add(self, request_id, embeds, max_tokens, eos=(), sampling=None, rules=None, prompt_ids=None):
        """sampling: None (greedy) or the keywords of MixtralEngine.seq_set_sampling without draw0 (see sampling_of).
        rules: None or the keywords of MixtralEngine.seq_set_logit_rules without the ids (see rules_of); prompt_ids: the prompt set
        of the penalties.  The rules are re-armed with prompt and output ids after a recompute preemption, and the logprobs of a
        request (self.logprobs[request_id]) run on across it."""
        S = int(embeds.shape[0])
        if S + 2 > self.eng.max_ctx or S > self.eng.max_prefill:
            raise ValueError(f"prompt of {S} tokens exceeds the engine (max_prefill {self.eng.max_prefill}, pool "
                             f"{self.eng.max_ctx} tokens)")
        self.waiting.append(dict(id=request_id, emb=embeds, max_tokens=min(int(max_tokens), self.eng.max_new),
                                 eos=set(eos), out=[], seq=None, base=0, sampling=sampling, rules=rules,
                                 prompt_ids=list(prompt_ids or ())))
        if rules is not None and rules.get("logprobs", -1) >= 0:
            self.logprobs[request_id] = []

    def abort(self, request_id):
        self.logprobs.pop(request_id, None)
        self.cached_tokens.pop(request_id, None)
        for r in list(self.running):
            if r["id"] == request_id:
                self._register_written(r)
                self.eng.seq_free(r["seq"])
                self.running.remove(r)
                return True
        for r in list(self.waiting):
            if r["id"] == request_id:
                self.waiting.remove(r)
                return True
        return False

    def has_work(self):
        return bool(self.waiting or self.running)

    def _pages(self, n_tokens):
        return -(-int(n_tokens) // 64)

    def _prefill(self, r):
        """the prompt of a request — or, after a preemption, prompt + generated tokens, which may exceed what one prefill call
        takes — in chunks of max_prefill (seq_prefill appends at the sequence's position)."""
        emb, mp = self._suffix(r), int(self.eng.max_prefill)
        for s0 in range(0, int(emb.shape[0]), mp):
            if s0 > 0 and s0 + mp >= int(emb.shape[0]):
                self._arm(r)                 # a chunked re-prompt: only the LAST chunk's token is an output (the table counts it)
            self.eng.seq_prefill(r["seq"], emb[s0:s0 + mp])
            self.stats["prefill_calls"] += 1
            self.stats["prefill_rows"] += int(emb[s0:s0 + mp].shape[0])

    def _suffix(self, r):
        """the rows of r's prompt that are prefilled: all of them, or what lies behind the pages it adopted."""
        hit = r.get("hit", 0)
        return r["emb"][64 * hit:] if hit else r["emb"]

    # ---- prefix cache ----------------------------------------------------------------------------------------------------------
    def _lookup(self, r):
        """keys of r's complete prompt blocks (hashed once per prompt; a re-prompt after a preemption only grew) -> the cached pages
        r may adopt, pinned until the admission pass ends."""
        c, S = self.cache, int(r["emb"].shape[0])
        keys = r.setdefault("keys", [])
        if len(keys) < S // 64:
            keys += c.keys_after(keys, r["emb"][64 * len(keys):])
        pages = c.match(keys, (S - 1) // 64)
        c.pinned.update(pages)
        return pages

    def _register(self, r, n_full):
        """hold r's first n_full pages for the cache, as far as their keys are not cached yet (those form the tail of the chain)."""
        c, keys = self.cache, r["keys"]
        new = [b for b in range(min(n_full, len(keys))) if keys[b] not in c.entries]
        if not new:
            return
        pages = self.eng.seq_hold_prefix(r["seq"], new[-1] + 1)
        if new[0] > 0:
            self.eng.pages_release(pages[:new[0]])             # the hold covers the table's head: the cached part goes back
        for b in new:
            c.insert(keys[b], keys[b - 1] if b else None, pages[b])

    def _register_written(self, r, rows=None):
        """before r's sequence is freed: register its pages that lie entirely below its position, those filled by generated tokens
        included.  rows: r's prompt + embed_tokens(its output), when the caller has built it anyway (preemption)."""
        if self.cache is None or self.embed_tokens is None or r.get("seq") is None:
            return
        S, keys = int(r["emb"].shape[0]), r.setdefault("keys", [])
        gen = r["out"][r["base"]:]
        # K/V of position S + i is the row of generated token i; the last accepted token was never fed (or its row is discarded)
        valid = min(self.eng.seq_pos(r["seq"]), S + max(len(gen) - 1, 0))
        if valid // 64 > len(keys):
            k0 = 64 * len(keys)
            if rows is None:
                tail = self.embed_tokens(torch.tensor(gen[:-1], dtype=torch.long, device=r["emb"].device)).to(torch.float32)
                rows = torch.cat([r["emb"][k0:], tail], dim=0)
            else:
                rows = rows[k0:]
            keys += self.cache.keys_after(keys, rows[:64 * (valid // 64) - k0])
        self._register(r, valid // 64)

    def _make_room(self, short):
        """the pool is `short` pages short: evict that many cached pages if the cache can -> True when it could."""
        if short <= 0:
            return True
        if self.cache is None or self.cache.evictable() < short:
            return False
        self.stats["prefix_evictions"] += self.cache.evict(short)
        return True

    def _arm(self, r):
        """the logit rules of r's slot with its history: the prompt set, and every token generated so far as outputs."""
        if r.get("rules") is not None:
            self.eng.seq_set_logit_rules(r["seq"], prompt_ids=r["prompt_ids"], output_ids=r["out"], **r["rules"])

    def _fail(self, r, exc, events):
        """ONE request failed (its prompt does not fit, its prefill was rejected): it ends with an "error" event, nobody else
        is touched.  Device-level failures (spin time-outs, launch errors seen at the synchronisation) still propagate."""
        self.errors[r["id"]] = exc
        self.logprobs.pop(r["id"], None)
        self.cached_tokens.pop(r["id"], None)
        self.stats["failed"] += 1
        events.append((r["id"], [], True, "error"))

    def _start(self, r, events, prefilled=False):
        """r holds a slot: prefill it (unless a group call already did) and let it run; a failure ends r alone."""
        if not prefilled:
            try:
                self._prefill(r)
            except Exception as e:
                self.eng.seq_free(r["seq"])
                r["seq"] = None
                self._fail(r, e, events)
                return
        r["fresh"] = True                    # its first token (tokens[0]) is not reported yet
        self.running.append(r)
        self.stats["prefills"] += 1
        if self.cache is not None:           # the prefill is enqueued: its full prompt pages can be shared from here on
            self._register(r, int(r["emb"].shape[0]) // 64)

    def _prefill_group(self, group, events):
        """the admitted requests of one group, in admission order: two or more in one pass over the weights.  A group call that
        raises is retried request by request (a rejected call touched nothing; after a later failure seq_prefill starts again
        at the sequence's unchanged position), so only the culprit ends with an "error" event."""
        done = False
        if len(group) >= 2:
            try:
                self.eng.seq_prefill_batch([r["seq"] for r in group], [self._suffix(r) for r in group])
                self.stats["prefill_calls"] += 1
                self.stats["prefill_rows"] += sum(int(self._suffix(r).shape[0]) for r in group)
                done = True
            except Exception:
                done = False
        for r in group:
            self._start(r, events, prefilled=done)
        group.clear()

    def _admit(self):
        events = []
        mp = int(self.eng.max_prefill)
        can_batch = hasattr(self.eng, "seq_prefill_batch")
        group, rows = [], 0       # admitted (slot taken, pages promised), prefill deferred to the group's call
        while self.waiting and len(self.running) + len(group) < self.max_batch:
            r = self.waiting[0]
            # the pool as it will be once the group is prefilled: the pages promised to its prompts are gone, its members run
            # (pages a member adopted from the prefix cache are in its table already)
            free = self.eng.pages_free() - sum(self._pages(g["emb"].shape[0]) - g.get("hit", 0) for g in group)
            n_run = len(self.running) + len(group)
            need = self._pages(r["emb"].shape[0] + 1) + n_run                   # + one page of headroom per runner
            hit = []
            if self.cache is not None:
                self.cache.tick += 1
                hit = self._lookup(r)
                need -= len(hit)
                if not self._make_room(need - free):        # free + evictable - promised; the pinned pages are not evictable
                    self.cache.pinned.difference_update(hit)
                else:
                    free = max(free, need)
            if need > free:
                if n_run == 0:
                    self.waiting.popleft()
                    self._fail(r, RuntimeError(f"request {r['id']}: prompt needs {need} KV pages, the pool has "
                                               f"{free}"), events)
                    continue
                break
            self.waiting.popleft()
            try:
                r["seq"] = self.eng.seq_alloc()
            except Exception as e:
                self._fail(r, e, events)
                continue
            if self.cache is not None:
                r["hit"] = len(hit)
                self.stats["prefix_queries"] += 1
                self.stats["prefix_hit_tokens"] += 64 * len(hit)
                self.cached_tokens.setdefault(r["id"], 64 * len(hit))
                if hit:
                    try:
                        self.eng.seq_adopt(r["seq"], hit)
                    except Exception as e:
                        self.eng.seq_free(r["seq"])
                        r["seq"] = None
                        self._fail(r, e, events)
                        continue
            if r["sampling"] is not None:
                # draw index of the next token = tokens already generated (r["base"] after a recompute preemption): the
                # continued ids are the ones an unpreempted run draws
                try:
                    self.eng.seq_set_sampling(r["seq"], draw0=r["base"], **r["sampling"])
                except Exception as e:
                    self.eng.seq_free(r["seq"])
                    r["seq"] = None
                    self._fail(r, e, events)
                    continue
            S = int(r["emb"].shape[0]) - 64 * r.get("hit", 0)     # the rows that are prefilled
            if S <= mp:                          # (a chunked re-prompt arms its rules in front of its last chunk: _prefill)
                try:
                    self._arm(r)
                except Exception as e:
                    self.eng.seq_free(r["seq"])
                    r["seq"] = None
                    self._fail(r, e, events)
                    continue
            if not can_batch or S > mp:          # no batched entry point / a re-prompt that goes in chunks: alone, in order
                self._prefill_group(group, events)
                rows = 0
                self._start(r, events)
                continue
            if rows + S > mp:                    # the next prompt would take the group's rows past max_prefill: close it
                self._prefill_group(group, events)
                rows = 0
            group.append(r)
            rows += S
        self._prefill_group(group, events)
        if self.cache is not None:
            self.cache.pinned.clear()
        return events

    def _preempt_for(self, steps):
        """make sure `steps` decode steps of every running sequence find their pages; youngest sequences yield."""
        while True:
            new_pages = sum(self._pages(self.eng.seq_pos(r["seq"]) + steps) - len(self.eng.seq_pages(r["seq"]))
                            for r in self.running)
            short = new_pages - self.eng.pages_free()
            if short > 0 and self.cache is not None:              # cached pages yield before a running sequence does
                self.stats["prefix_evictions"] += self.cache.evict(short)
                short = new_pages - self.eng.pages_free()
            if short <= 0 or len(self.running) <= 1:
                return
            r = self.running.pop()
            keep = self.cache is not None and self.embed_tokens is not None   # register its written pages before they are freed
            if not keep:
                self.eng.seq_free(r["seq"])
            if r["out"] and self.embed_tokens is None:
                raise RuntimeError("KV pool exhausted and no embed_tokens hook to recompute a preempted sequence")
            emb = r["emb"]
            if r["out"][r["base"]:]:
                tail = self.embed_tokens(torch.tensor(r["out"][r["base"]:], dtype=torch.long, device=r["emb"].device))
                emb = torch.cat([r["emb"], tail.to(torch.float32)], dim=0)
            if keep:                                              # its written pages stay findable: the re-prompt adopts them
                self._register_written(r, rows=emb)
                self.eng.seq_free(r["seq"])
            r["emb"] = emb
            r["base"], r["seq"] = len(r["out"]), None
            self.waiting.appendleft(r)
            self.stats["preemptions"] += 1

    @torch.no_grad()
    def step(self):
        failed = self._admit()
        if not self.running:
            return failed
        # decode window, bounded by every sequence's token buffer and by the pool's addressable context
        steps = self.window
        for r in self.running:
            n_dev = len(r["out"]) - r["base"] + (1 if r.get("fresh") else 0)
            steps = min(steps, self.eng.max_new - n_dev, self.eng.max_ctx - 2 - self.eng.seq_pos(r["seq"]))
        steps = max(steps, 0)
        starved = None
        if steps > 0:
            self._preempt_for(steps)
            if len(self.running) == 1:
                r = self.running[0]
                if self._pages(self.eng.seq_pos(r["seq"]) + steps) - len(self.eng.seq_pages(r["seq"])) > self.eng.pages_free():
                    starved, steps = r, 0                         # alone and the pool is dry: it ends here ("length")
        if steps > 0:
            ids = [r["seq"] for r in self.running]
            for _ in range(steps):
                self.eng.seq_decode(ids)
            self.stats["decode_steps"] += steps * len(ids)
        self.stats["iterations"] += 1
        torch.cuda.current_stream().synchronize()
        events = failed
        for r in list(self.running):
            cnt = self.eng.check_device_flag(self.eng.seq_counters(r["seq"]).tolist())
            n_dev = min(cnt[1], self.eng.max_new)                 # tokens of this (re)prefill + its decode steps
            have = len(r["out"]) - r["base"]
            new = self.eng.seq_tokens(r["seq"])[have:n_dev].tolist()
            new_lp = None
            if r["id"] in self.logprobs and n_dev > have:
                from .model.vita_mixtral import logprob_dicts
                views = self.eng.logprobs(r["seq"])
                new_lp = logprob_dicts(tuple(v[have:n_dev] for v in views), new, r["rules"]["logprobs"])
            r["fresh"] = False
            accepted, reason = [], None
            for tok in new:
                accepted.append(tok)
                if tok in r["eos"]:
                    reason = "stop"
                elif len(r["out"]) + len(accepted) >= r["max_tokens"]:
                    reason = "length"
                if reason:
                    break
            r["out"] += accepted
            if new_lp is not None:
                self.logprobs[r["id"]] += new_lp[:len(accepted)]
            if reason is None and (r is starved or self.eng.seq_pos(r["seq"]) + 2 >= self.eng.max_ctx):
                reason = "length"                                 # the pool cannot hold another token of this sequence
            if reason:
                self._register_written(r)
                self.eng.seq_free(r["seq"])
                self.running.remove(r)
            if accepted or reason:
                events.append((r["id"], accepted, reason is not None, reason or ""))
        return events


@dataclass
class AsyncEngineArgs:
    """the fields web_interactive_demo.py:942-951 sets, plus the scheduler's knobs (vLLM names)."""
    model: str = ""
    dtype: str = "float16"
    tensor_parallel_size: int = 1
    trust_remote_code: bool = True
    gpu_memory_utilization: float = 0.8
    disable_custom_all_reduce: bool = True
    limit_mm_per_prompt: Optional[dict] = None
    max_num_seqs: int = 8
    max_new_tokens: int = 1024
    kv_pool_tokens: Optional[int] = None     # size of the paged KV pool; default: max_num_seqs x (<= 1024-token prompt + max_new_tokens),
                                             # bounded by gpu_memory_utilization of the free memory (VITAMixtralForCausalLM.default_kv_pool_tokens)
    device: str = "cuda"
    quantization: Optional[str] = None       # None or "experts_int8" (LLM)
    max_logprobs: int = 0                    # > 0 (<= 20): SamplingParams' penalties and logprobs on the device (LLM)
    enable_prefix_caching: bool = False      # reuse the KV pages of earlier prompts with the same leading rows (ContinuousBatcher)


class AsyncLLMEngine:
    """`vllm.AsyncLLMEngine` as the interactive demo uses it (web_interactive_demo.py:126, 315-328):

        llm = AsyncLLMEngine.from_engine_args(AsyncEngineArgs(model=path, ...))
        async for request_output in llm.generate(inputs, sampling_params=sp, request_id=uuid):
            text = request_output.outputs[0].text          # cumulative

    Requests submitted while others are running are batched by `ContinuousBatcher`: one scheduler thread owns the GPU
    stream (encoders + prefill of admitted requests, then one decode step for every running sequence per iteration) and
    posts RequestOutputs to the callers' event loops."""

    def __init__(self, llm: "LLM", max_num_seqs=None, window=1, enable_prefix_caching=None):
        self.llm = llm
        eng = llm.model.engine
        if enable_prefix_caching is None:
            enable_prefix_caching = getattr(llm, "enable_prefix_caching", False)
        self.batcher = ContinuousBatcher(eng, embed_tokens=lambda ids: llm.model.model.embed_tokens(ids),
                                         max_batch=max_num_seqs, window=window, prefix_cache=bool(enable_prefix_caching))
        self._cache_resets = []           # threading.Event per pending reset_prefix_cache()
        self._lock = threading.Lock()
        self._cv = threading.Condition(self._lock)
        self._incoming, self._aborts, self._sinks = [], [], {}
        self._closed = False
        self._thread = threading.Thread(target=self._loop, daemon=True, name="vita-amd-scheduler")
        self._thread.start()

    @classmethod
    def from_engine_args(cls, args: AsyncEngineArgs, **kw):
        pool = args.kv_pool_tokens
        llm = LLM(args.model, dtype=args.dtype, tensor_parallel_size=args.tensor_parallel_size,
                  gpu_memory_utilization=args.gpu_memory_utilization,
                  limit_mm_per_prompt=args.limit_mm_per_prompt, max_new_tokens=args.max_new_tokens, device=args.device,
                  max_num_seqs=args.max_num_seqs, kv_pool_tokens=pool, quantization=args.quantization,
                  max_logprobs=args.max_logprobs, enable_prefix_caching=args.enable_prefix_caching)
        return cls(llm, max_num_seqs=args.max_num_seqs, **kw)

    def reset_prefix_cache(self, timeout=30.0):
        """drop every cached prefix (vLLM's name): done by the scheduler thread between two iterations; returns once it is done.
        Pages that running requests adopted stay theirs until they end.  -> True (False: no cache, or the scheduler did not answer)."""
        if self.batcher.cache is None:
            return False
        done = threading.Event()
        with self._cv:
            self._cache_resets.append(done)
            self._cv.notify()
        return done.wait(timeout)

    async def get_tokenizer(self):
        return self.llm.tokenizer

    # -- scheduler thread ----------------------------------------------------------------------------------------------
    def _post(self, rid, item):
        sink = self._sinks.get(rid)
        if sink is not None:
            loop, q = sink
            loop.call_soon_threadsafe(q.put_nowait, item)

    def _loop(self):
        if torch.cuda.is_available():
            torch.cuda.set_device(self.llm.model.device)      # kernels launch on the CURRENT device's stream
        state = {}                                   # request id -> (prompt ids, sampling params, token list)
        while True:
            with self._cv:
                while not (self._incoming or self._aborts or self._cache_resets or self.batcher.has_work() or self._closed):
                    self._cv.wait()
                if self._closed:
                    return
                incoming, self._incoming = self._incoming, []
                aborts, self._aborts = self._aborts, []
                resets, self._cache_resets = self._cache_resets, []
            if resets:
                self.batcher.cache.clear()
                for ev in resets:
                    ev.set()
            for rid in aborts:
                self.batcher.abort(rid)
                state.pop(rid, None)
            for rid, inputs, sp in incoming:
                try:
                    req = self.llm._prepare(inputs, sp)
                    emb = self.llm._embed(req)
                    self.batcher.add(rid, emb, req["max_tokens"], req["eos"], sampling=sampling_of(sp), rules=req.get("rules"),
                                     prompt_ids=req.get("prompt_set"))
                    state[rid] = (req["ids"], sp, [])
                except BaseException as e:          # surfaced to the caller's iterator
                    self._post(rid, e)
            try:
                events = self.batcher.step()
            except BaseException as e:
                for rid in list(state):
                    self._post(rid, e)
                state.clear()
                self.batcher.waiting.clear()
                self.batcher.logprobs.clear()
                for r in list(self.batcher.running):
                    self.batcher.abort(r["id"])
                continue
            for rid, new, finished, reason in events:
                if rid not in state:
                    continue
                if reason == "error":                # this request alone failed (ContinuousBatcher._fail)
                    self._post(rid, self.batcher.errors.pop(rid, RuntimeError(f"request {rid} failed")))
                    state.pop(rid)
                    continue
                ids, sp, toks = state[rid]
                toks += new
                text = self.llm.tokenizer.decode(toks, skip_special_tokens=sp.skip_special_tokens)
                lps = self.batcher.logprobs.pop(rid, None) if finished else self.batcher.logprobs.get(rid)
                cached = self.batcher.cached_tokens.pop(rid, 0) if finished else self.batcher.cached_tokens.get(rid, 0)
                self._post(rid, RequestOutput(request_id=str(rid), prompt_token_ids=ids, finished=finished,
                                              outputs=[completion(0, text, list(toks), reason, lps)], num_cached_tokens=cached))
                if finished:
                    state.pop(rid)

    # -- caller side -----------------------------------------------------------------------------------------------------
    async def generate(self, inputs, sampling_params: SamplingParams = None, request_id=None, **_):
        sp = sampling_params or SamplingParams()
        rid = request_id if request_id is not None else os.urandom(8).hex()
        q = asyncio.Queue()
        with self._cv:
            if rid in self._sinks:
                raise ValueError(f"request id {rid!r} is already running")
            self._sinks[rid] = (asyncio.get_running_loop(), q)
            self._incoming.append((rid, inputs, sp))
            self._cv.notify()
        try:
            while True:
                item = await q.get()
                if isinstance(item, BaseException):
                    raise item
                yield item
                if item.finished:
                    return
        finally:
            with self._cv:
                self._sinks.pop(rid, None)
                self._aborts.append(rid)          # a consumer that leaves early (interrupt, noise verdict) frees the pages
                self._cv.notify()

    async def abort(self, request_id):
        with self._cv:
            self._aborts.append(request_id)
            self._cv.notify()

    def shutdown(self):
        with self._cv:
            self._closed = True
            self._cv.notify()
        self._thread.join(timeout=30)
