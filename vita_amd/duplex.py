"""Duplex two-engine serving (BASELINE configs[4]) — the orchestration of the reference's
web_demo/web_interactive_demo.py:105-379,911-1029, without its Gradio / VAD / TTS front ends.

Two identical engines (replicas: no tensor traffic between them) alternate between two roles:

  * whoever holds the `start` baton takes the next request from the shared input queue and immediately hands
    the baton to the other engine (web_interactive_demo.py:284-293) — so a new query that arrives while this
    engine is still speaking is picked up by the other one ("monitor");
  * an engine streams its answer; if the first generated text starts with the state token `<2>` the query is
    classed as noise and dropped silently (:221-223,368-370); otherwise, on its FIRST positive chunk it clears its
    own stop flag, raises the OTHER engine's stop flag and clears the output queue (:340-352) — the monitor
    interrupts the generator;
  * an engine polls its own stop flag between decode windows and abandons its answer when it is set (:354-366);
  * finished sentences (split on punctuation) go to the output queue, the finished turn to the shared history.

Conversation mode (`conversation=True`, off by default): a turn is answered with the last `history_turns` finished turns in
its prompt (`merge_current_and_history`, web_interactive_demo.py:297-302, 604-680) — the history's audio clips stay in
`multi_modal_data` ahead of the current clip, its images are dropped — and the merged prompt is re-tokenised with the engine's
placeholder ids (:308).  The history keeps the UNMERGED request: prompt, multi_modal_data, response.

`worker_loop` is the per-engine process body; it only needs an object with
`generate_stream(inputs, sampling_params, request_id, should_stop) -> iterator of RequestOutput` (vita_amd.serving.LLM
has it), so the protocol is unit-tested on the CPU with scripted engines and on the GPU with two real engines.
`DuplexServer` wires two worker processes with multiprocessing primitives, one process per engine."""
import multiprocessing as mp
import queue as _queue
import time
import uuid

from .host.prompt import SYSTEM_PROMPTS, tokenizer_image_audio_token

NEGATIVE_PREFIX = "<2>"
SENTENCE_END = [",", "，", ".", "。", "?", "\n", "？", "!", "！", "、"]
IMAGE_TOKEN, VIDEO_TOKEN = "<image>", "<video>"
USER_PREFIX, BOT_PREFIX, TURN_END = "user:", "bot:", "</s>\n"
MODALITIES = ("image", "audio", "video")


def demo_system_prompt(request):
    """The interactive demo's system block for a request (web_interactive_demo.py:611-627): the media prompt — the VIDEO
    one for an image as well — or the plain one; the demo spells the model's name "Vita" where the offline templates
    (host/prompt.py) say "VITA", otherwise the strings are the same."""
    mm = request.get("multi_modal_data") or {}
    which = 1 if ("video" in mm or "image" in mm) else 2
    return "system:" + SYSTEM_PROMPTS[which].replace("your name is VITA", "your name is Vita", 1) + TURN_END


def _strip_state_space(text):
    return text.replace("<1> ", "<1>").replace("<2> ", "<2>")


def merge_current_and_history(history, request, skip_history_vision=False, move_image_token_to_start=False):
    """The prompt and modal data of `request` with the turns of `history` in front (web_interactive_demo.py:604-680; same
    results).  `request` is updated in place and returned, as the reference does.  history entries: {"prompt", "response"[,
    "multi_modal_data"]}.  An empty history only frames the prompt and leaves the modal data alone."""
    system = demo_system_prompt(request)
    ask = USER_PREFIX + request["prompt"] + TURN_END + BOT_PREFIX
    if len(history) == 0:
        request["prompt"] = _strip_state_space(system + ask)
        return request
    text, data = system, {m: [] for m in MODALITIES}
    kept = [m for m in MODALITIES if not (skip_history_vision and m in ("image", "video"))]
    for turn in history:
        if "prompt" not in turn or "response" not in turn:
            raise AssertionError("a history turn needs its prompt and its response")
        said = turn["prompt"]
        if skip_history_vision:
            said = said.replace(IMAGE_TOKEN, "").replace(VIDEO_TOKEN, "")
        text += USER_PREFIX + said + TURN_END + BOT_PREFIX + turn["response"] + TURN_END
        for m in kept:
            data[m].extend((turn.get("multi_modal_data") or {}).get(m, []))
    text += ask
    for m in MODALITIES:
        data[m].extend((request.get("multi_modal_data") or {}).get(m, []))
    data = {m: v for m, v in data.items() if len(v)}
    if move_image_token_to_start:
        n = text.count(IMAGE_TOKEN)
        body = text.replace(IMAGE_TOKEN, "").replace(system, "")
        # str.lstrip takes a character SET: like the reference, this also eats leading letters of the first words that are in "user:"
        text = system + USER_PREFIX + IMAGE_TOKEN * n + body.lstrip(USER_PREFIX)
    request["prompt"] = _strip_state_space(text)
    request["multi_modal_data"] = data
    return request


def conversation_inputs(llm, history, request, history_turns=1):
    """What a conversation-mode turn hands to the engine: `request` merged with the last `history_turns` turns (history vision
    skipped, image tokens moved to the start: web_interactive_demo.py:297-302) and, when the engine has a tokenizer, the
    merged prompt as `prompt_token_ids` with the engine's placeholder ids (:308).  `request` itself is not modified."""
    turns = list(history)[-int(history_turns):] if int(history_turns) > 0 else []
    merged = dict(request)
    if "multi_modal_data" in merged:
        merged["multi_modal_data"] = {k: list(v) if isinstance(v, (list, tuple)) else [v]
                                      for k, v in merged["multi_modal_data"].items()}
    merged = merge_current_and_history(turns, merged, skip_history_vision=True, move_image_token_to_start=True)
    tok = getattr(llm, "tokenizer", None)
    if tok is not None and "prompt" in merged:
        merged["prompt_token_ids"] = tokenizer_image_audio_token(
            merged["prompt"], tok, image_token_index=int(getattr(llm, "image_token_index", 51000)),
            audio_token_index=int(getattr(llm, "audio_token_index", 51001)))
    return merged


def judge_negative(text):
    return text.startswith(NEGATIVE_PREFIX)          # web_interactive_demo.py:221-223


def clear_queue(q):
    while True:
        try:
            q.get_nowait()
        except _queue.Empty:
            return


def worker_loop(llm_id, make_llm, sampling_params, inputs_queue, outputs_queue, stop_event, other_stop_event,
                worker_ready, wait_workers_ready, start_event, other_start_event, start_event_lock, interrupt_signal,
                global_history, shutdown_event, stats_queue=None, history_limit=0, poll_s=0.005, conversation=False,
                history_turns=1):
    """Body of one engine process (web_interactive_demo.py:105-379).  conversation=True: every turn is merged with the last
    `history_turns` history entries before it reaches the engine (conversation_inputs); off, the engine receives exactly what
    was submitted."""
    llm = make_llm()
    worker_ready.set()
    while not shutdown_event.is_set():
        if not all(w.is_set() for w in wait_workers_ready):
            time.sleep(poll_s)
            continue
        if inputs_queue.empty():
            time.sleep(poll_s)
            continue
        with start_event_lock:
            if not start_event.is_set():
                continue
            try:
                inputs = inputs_queue.get_nowait()
            except _queue.Empty:
                continue
            other_start_event.set()                   # hand the baton over before starting to work
            start_event.clear()
        t_take = time.perf_counter()
        current = dict(inputs)
        error = None
        if conversation:
            try:
                inputs = conversation_inputs(llm, global_history, current, history_turns)
            except Exception as e:     # a malformed request is answered like a failed one below; the baton was already passed on
                error = f"{type(e).__name__}: {e}"
                print(f"[duplex worker {llm_id}] request failed: {error}", flush=True)
                if stats_queue is not None:
                    stats_queue.put({"id": llm_id, "request": current.get("request_id"), "take_to_first_chunk_s": None,
                                     "first_chunk_to_end_s": None, "n_tokens": 0, "interrupted": False, "negative": True,
                                     "n_chunks": 0, "error": error})
                continue
        results, pending, first_positive, t_first = [], "", True, None
        previous, n_tokens = "", 0
        st = {"speaking": False}     # the stop flag only counts once this engine has taken the floor (:354)
        stream = llm.generate_stream(inputs, sampling_params, request_id=uuid.uuid4().hex,
                                     should_stop=lambda: st["speaking"] and stop_event.is_set())
        try:
            for out in stream:
                text = out.outputs[0].text
                n_tokens = len(out.outputs[0].token_ids)
                new = text[len(previous):]
                previous = text
                if new == "":
                    continue
                if t_first is None:
                    t_first = time.perf_counter()
                if judge_negative(new) or (first_positive and judge_negative(text)):
                    break                                   # noise: answer nothing
                pending += new
                if first_positive:                          # first real words: take the floor
                    stop_event.clear()
                    other_stop_event.set()
                    clear_queue(outputs_queue)
                    first_positive = False
                    st["speaking"] = True
                    interrupt_signal.value = llm_id
                if stop_event.is_set():
                    break                                   # the other engine took the floor
                results.append(new)
                pending = pending.replace("<1> ", "").replace("<1>", "")
                if new in SENTENCE_END or new[-1:] in SENTENCE_END:
                    outputs_queue.put({"id": llm_id, "response": pending})
                    pending = ""
        except Exception as e:      # one bad request must not kill the engine process: the baton would never return
            error = f"{type(e).__name__}: {e}"
            print(f"[duplex worker {llm_id}] request failed: {error}", flush=True)
        finally:
            stream.close()            # abandons the generation (noise verdict / interrupt / error) without decoding on
        if pending and not stop_event.is_set() and not first_positive:
            outputs_queue.put({"id": llm_id, "response": pending})
        current["response"] = "".join(results)
        if current["response"]:
            keep = ("prompt", "response", "multi_modal_data") if conversation else ("prompt", "response")
            global_history.append({k: v for k, v in current.items() if k in keep})
            if history_limit and len(global_history) > history_limit:
                del global_history[0]
        if stats_queue is not None:
            t_end = time.perf_counter()
            stats_queue.put({"id": llm_id, "request": current.get("request_id"),
                             "take_to_first_chunk_s": None if t_first is None else t_first - t_take,
                             "first_chunk_to_end_s": None if t_first is None else t_end - t_first, "n_tokens": n_tokens,
                             "interrupted": bool(stop_event.is_set()), "negative": first_positive,
                             "n_chunks": len(results), "error": error})


def _engine_process(llm_id, llm_factory, factory_args, sampling_params, shared, engines_share_device=True):
    if engines_share_device:
        # two replicas on ONE GPU: launches whose blocks wait for other blocks (the fused decode attention block) can be starved by the
        # other replica's waiting blocks — the library keeps the three-launch form for processes that share a device
        from . import _lib
        _lib.tune("comm_ranks_per_device", 2)
    worker_loop(llm_id, lambda: llm_factory(*factory_args), sampling_params, **shared)


class DuplexServer:
    """Two engine processes + the shared queues / events of web_interactive_demo.py:914-1029."""

    def __init__(self, llm_factory, factory_args=(), sampling_params=None, history_limit=0, ctx="spawn", engines_share_device=True,
                 conversation=False, history_turns=1):
        """conversation / history_turns: answer every turn with the last `history_turns` finished turns in its prompt (worker_loop).
        engines_share_device: the two replicas drive the same GPU (the default assumption; pass False when the factory places
        them on different devices, as the reference's demo does: cuda_devices "0,1" / "2,3", web_interactive_demo.py:958,981)."""
        self.mpc = mp.get_context(ctx)
        self.mgr = self.mpc.Manager()
        m = self.mgr
        self.inputs, self.outputs, self.stats = m.Queue(), m.Queue(), m.Queue()
        self.history = m.list()
        self.shutdown = m.Event()
        self.lock = m.Lock()
        self.interrupt = m.Value("i", -1)
        ready = [m.Event(), m.Event()]
        stop = [m.Event(), m.Event()]
        start = [m.Event(), m.Event()]
        start[0].set()                                  # engine 0 holds the baton first (:1010)
        self.procs = []
        for i in range(2):
            shared = dict(inputs_queue=self.inputs, outputs_queue=self.outputs, stop_event=stop[i],
                          other_stop_event=stop[1 - i], worker_ready=ready[i], wait_workers_ready=ready,
                          start_event=start[i], other_start_event=start[1 - i], start_event_lock=self.lock,
                          interrupt_signal=self.interrupt, global_history=self.history,
                          shutdown_event=self.shutdown, stats_queue=self.stats, history_limit=history_limit)
            if conversation:
                shared.update(conversation=True, history_turns=int(history_turns))
            p = self.mpc.Process(target=_engine_process, args=(i, llm_factory, factory_args, sampling_params, shared, engines_share_device),
                                 daemon=True)
            p.start()
            self.procs.append(p)
        # keep the parent's proxies alive: a Manager drops an object whose last proxy is collected, and the
        # spawned children attach seconds later
        self._ready, self._stop, self._start = ready, stop, start

    def wait_ready(self, timeout=600):
        t0 = time.time()
        while not all(e.is_set() for e in self._ready):
            if time.time() - t0 > timeout or any(not p.is_alive() for p in self.procs):
                raise RuntimeError("duplex engines failed to start")
            time.sleep(0.05)

    def submit(self, inputs):
        self.inputs.put(dict(inputs))

    def close(self):
        self.shutdown.set()
        for p in self.procs:
            p.join(timeout=10)
            if p.is_alive():
                p.terminate()
        self.mgr.shutdown()


def make_serving_llm(model_path, max_new_tokens=128, max_logprobs=0):
    """Default engine factory of a worker process: one vita_amd.serving.LLM replica on the visible GPU.  max_logprobs > 0 (e.g.
    factory_args=(path, 128, 20)) creates the token tables and logprob buffers that SamplingParams' penalties and logprobs need;
    without it a turn that asks for them raises ValueError."""
    from .serving import LLM
    return LLM(model=model_path, tensor_parallel_size=1, max_new_tokens=max_new_tokens, max_logprobs=max_logprobs)
