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
include/vita_hip.h); `ContinuousBatcher` (vita_amd/scheduler.py) is the iteration-level scheduler over it (admit -> prefill, one
decode step for every running sequence per iteration, free on finish, preempt-by-recompute when the pool runs dry) and
`AsyncLLMEngine.generate(inputs, sampling_params, request_id)` is the async iterator the demo consumes.  `LLM.generate`
(the offline demo) keeps serving one request at a time on the same engine."""
import asyncio
import contextlib
import json
import os
import queue
import threading
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from .host.constants import AUDIO_TOKEN_INDEX, IMAGE_TOKEN_INDEX
from .host.image_processing import dynamic_preprocess
from .scheduler import PREFIX_ROOT_KEY, ContinuousBatcher, PrefixCache, Request, chain_keys, device_digests   # noqa: F401  (re-exported)


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
                 enable_prefix_caching=False, enable_chunked_prefill=False, max_num_batched_tokens=None, **_):
        from .model.builder import load_pretrained_model
        # vLLM's switch: AsyncLLMEngine's batcher then keeps finished prompts' KV pages under content keys (PrefixCache).  generate()
        # here serves one request at a time on the contiguous pool and does not use the cache; the engine refuses it while the cache
        # holds pages (its error names reset_prefix_cache)
        self.enable_prefix_caching = bool(enable_prefix_caching)
        # vLLM's switches: AsyncLLMEngine's batcher then runs prompt chunks and the running sequences' decode steps in one pass over the
        # weights, at most max_num_batched_tokens rows per pass (ContinuousBatcher chunked_prefill; default: the engine's max_prefill)
        self.enable_chunked_prefill = bool(enable_chunked_prefill)
        self.max_num_batched_tokens = max_num_batched_tokens
        # vLLM's quantization="experts_int8": the MoE experts as int8 with per-output-row scales
        # "experts_mxfp4": the experts as OCP MXFP4 (e2m1 codes, one power-of-two scale per 32 weights)
        if quantization not in (None, "experts_int8", "experts_mxfp4"):
            raise ValueError(f"quantization={quantization!r}: vita_amd supports None, 'experts_int8' and 'experts_mxfp4'")
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
            torch.cuda.set_device(torch.device(device))       # kernels launch on the CURRENT device's stream
        self.tokenizer, self.model, self.image_processor, _ = load_pretrained_model(
            model, None, os.path.basename(str(model).rstrip("/")), "mixtral-8x7b", device=device,
            max_new_tokens=max_new_tokens, max_seqs=int(max_num_seqs), kv_pool_tokens=kv_pool_tokens,
            gpu_memory_utilization=gpu_memory_utilization, load_8bit=quantization == "experts_int8",
            experts_mxfp4=quantization == "experts_mxfp4",
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
                T = max(len(a) for a in audios)
                feats = torch.zeros((len(audios), T, audios[0].size(1)))
                for i, a in enumerate(audios):
                    feats[i, :len(a)] = a.float()
            else:
                feats = audios[0].float()[None]
            lens = torch.tensor([len(a) for a in audios])
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
            frames = [len(a) for a in audios]
            exp = expanded_token_ids(sent, frames, image_token_index=self.image_token_index, audio_token_index=self.audio_token_index)
            V = int(self.model.config.vocab_size)
            prompt_set = sorted({t for t in exp if 0 <= t < V})
        return dict(ids=ids, sent=sent, pix=pix, feats=feats.to(dev), lens=lens.to(dev), normalized=normalized,
                    max_tokens=max_tokens, eos=eos, rules=rules, prompt_set=prompt_set)

    @contextlib.contextmanager
    def _audio_input(self, normalized):
        """the audio encoder reads a prepared request's features as they are: CMVN-normalised already, or raw"""
        enc = self.model.get_audio_encoder()
        enc.normalized_input = normalized
        try:
            yield
        finally:
            enc.normalized_input = False

    @torch.no_grad()
    def _embed(self, req):
        """encoders + splice of a prepared request -> inputs_embeds [S, H] fp32 on the device."""
        dev = self.model.device
        with self._audio_input(req["normalized"]):
            out = self.model.prepare_inputs_labels_for_multimodal(
                torch.tensor([req["sent"]], dtype=torch.long, device=dev), None, None, None, None, req["pix"],
                {"audios": req["feats"], "lengths": req["lens"]}, audio_valid_rows=True)
        return out[4][0].to(torch.float32)

    @torch.no_grad()
    def _one(self, inp, sp: SamplingParams, streamer=None):
        req = self._prepare(inp, sp)
        ids, sent, pix, feats, lens, max_tokens = (req[k] for k in ("ids", "sent", "pix", "feats", "lens", "max_tokens"))
        dev = self.model.device
        rules = req.get("rules")
        rkw = {} if rules is None else dict(repetition_penalty=rules["repetition_penalty"], presence_penalty=rules["presence_penalty"],
                                             frequency_penalty=rules["frequency_penalty"], penalty_prompt_ids=req["prompt_set"],
                                             output_logprobs=rules["logprobs"] if rules["logprobs"] >= 0 else None)
        with self._audio_input(req["normalized"]):
            out = self.model.generate(torch.tensor([sent], dtype=torch.long, device=dev), images=pix,
                                      audios={"audios": feats.to(dev), "lengths": lens.to(dev)}, num_beams=1,
                                      return_dict_in_generate=True, max_new_tokens=max_tokens,
                                      eos_token_id=list(req["eos"]), streamer=streamer, audio_valid_rows=True,
                                      **sample_kwargs(sp), **rkw)
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
    quantization: Optional[str] = None       # None, "experts_int8" or "experts_mxfp4" (LLM)
    max_logprobs: int = 0                    # > 0 (<= 20): SamplingParams' penalties and logprobs on the device (LLM)
    enable_prefix_caching: bool = False      # reuse the KV pages of earlier prompts with the same leading rows (ContinuousBatcher)
    enable_chunked_prefill: bool = False     # prompt chunks and the running sequences' decode steps in ONE pass over the weights
    max_num_batched_tokens: Optional[int] = None   # rows of such a pass (default and upper bound: the engine's max_prefill)


class AsyncLLMEngine:
    """`vllm.AsyncLLMEngine` as the interactive demo uses it (web_interactive_demo.py:126, 315-328):

        llm = AsyncLLMEngine.from_engine_args(AsyncEngineArgs(model=path, ...))
        async for request_output in llm.generate(inputs, sampling_params=sp, request_id=uuid):
            text = request_output.outputs[0].text          # cumulative

    Requests submitted while others are running are batched by `ContinuousBatcher`: one scheduler thread owns the GPU
    stream (encoders + prefill of admitted requests, then one decode step for every running sequence per iteration) and
    posts RequestOutputs to the callers' event loops."""

    def __init__(self, llm: "LLM", max_num_seqs=None, window=1, enable_prefix_caching=None, enable_chunked_prefill=None,
                 max_num_batched_tokens=None):
        self.llm = llm
        eng = llm.model.engine
        if enable_prefix_caching is None:
            enable_prefix_caching = getattr(llm, "enable_prefix_caching", False)
        if enable_chunked_prefill is None:
            enable_chunked_prefill = getattr(llm, "enable_chunked_prefill", False)
        if max_num_batched_tokens is None:
            max_num_batched_tokens = getattr(llm, "max_num_batched_tokens", None)
        self.batcher = ContinuousBatcher(eng, embed_tokens=lambda ids: llm.model.model.embed_tokens(ids),
                                         max_batch=max_num_seqs, window=window, prefix_cache=bool(enable_prefix_caching),
                                         chunked_prefill=bool(enable_chunked_prefill), max_batched_tokens=max_num_batched_tokens)
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
                  max_logprobs=args.max_logprobs, enable_prefix_caching=args.enable_prefix_caching,
                  enable_chunked_prefill=args.enable_chunked_prefill, max_num_batched_tokens=args.max_num_batched_tokens)
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
                for r in (*self.batcher.running, *self.batcher.waiting):      # nothing of this iteration can be trusted
                    self.batcher.abort(r.id)
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
