"""Conversation mode of the duplex server on the CPU: `merge_current_and_history` against the reference's own function
(web_demo/web_interactive_demo.py:604-680, cut out of its file; skipped where the reference tree is absent) and against cases
evaluated by hand, then the turn protocol on scripted engines that record the `inputs` they receive — the second turn must see
the merged prompt and [history clip, current clip], a noise turn leaves no history, history_turns bounds the memory, and with
conversation off the engine receives exactly what was submitted."""
import contextlib
import copy
import io
import itertools
import os
import threading
import time
from types import SimpleNamespace

import pytest

from oracle import ref_harness
from vita_amd import duplex
from vita_amd.duplex import merge_current_and_history

SYS_PLAIN = ("system:You are an AI robot and your name is Vita. \n- You are a multimodal large language model developed by the open "
             "source community. Your aim is to be helpful, honest and harmless. \n- You support the ability to communicate "
             "fluently and answer user questions in multiple languages of the user's choice. \n- If the user corrects the wrong "
             "answer you generated, you will apologize and discuss the correct answer with the user.</s>\n")
VIDEO_TAIL = (" \n- You must answer the question strictly according to the content of the video given by the user, and it is "
              "strictly forbidden to answer the question without the content of the video. Please note that you are seeing the "
              "video, not the image.</s>\n")
SYS_VIDEO = SYS_PLAIN[:-len("</s>\n")] + VIDEO_TAIL

H_AUDIO = {"prompt": "<audio>", "response": "<1> hello there.", "multi_modal_data": {"audio": ["A0"]}}
H_IMAGE = {"prompt": "<image><audio>", "response": "<2> nothing", "multi_modal_data": {"audio": ["A1"], "image": ["I1"]}}
H_VIDEO = {"prompt": "<video>sure?", "response": "use it", "multi_modal_data": {"video": ["V1"]}}
H_TEXT = {"prompt": "plain words", "response": "<1> plain answer"}
REQUESTS = [
    {"prompt": "hi"},
    {"prompt": "<audio>", "multi_modal_data": {"audio": ["A9"]}},
    {"prompt": "<image><audio>", "multi_modal_data": {"image": ["I9"], "audio": ["A9"]}},
    {"prompt": "<image>user says", "multi_modal_data": {"image": ["I9"]}},
    {"prompt": "<video>what", "multi_modal_data": {"video": ["V9"]}},
    {"prompt": "x", "multi_modal_data": {}},
]
HISTORIES = [[], [H_AUDIO], [H_AUDIO, H_IMAGE], [H_IMAGE, H_VIDEO], [H_VIDEO], [H_TEXT, H_AUDIO]]


@pytest.mark.skipif(not ref_harness.available(), reason="reference tree absent")
def test_merge_equals_the_reference_function():
    path = os.path.join(ref_harness.REF, "web_demo", "web_interactive_demo.py")
    ref = ref_harness.extract_functions(path, ["merge_current_and_history"])["merge_current_and_history"]
    ref.__globals__["IMAGE_TOKEN"], ref.__globals__["VIDEO_TOKEN"] = "<image>", "<video>"
    n = 0
    for hist, req in itertools.product(HISTORIES, REQUESTS):
        for skip, move in itertools.product((False, True), (False, True)):
            with contextlib.redirect_stdout(io.StringIO()):          # the reference prints the request
                want = ref(copy.deepcopy(hist), copy.deepcopy(req), skip, move)
            got = merge_current_and_history(copy.deepcopy(hist), copy.deepcopy(req), skip, move)
            assert got == want, (hist, req, skip, move)
            n += 1
    assert n == len(HISTORIES) * len(REQUESTS) * 4


def test_merge_cases_evaluated_by_hand():
    # empty history: only the frame; the modal data is left alone (not even normalised)
    r = merge_current_and_history([], {"prompt": "hi <1> x"}, True, True)
    assert r == {"prompt": SYS_PLAIN + "user:hi <1>x</s>\nbot:"}
    r = merge_current_and_history([], {"prompt": "<image>see", "multi_modal_data": {"image": ["I"], "video": []}})
    assert r == {"prompt": SYS_VIDEO + "user:<image>see</s>\nbot:", "multi_modal_data": {"image": ["I"], "video": []}}   # an image takes the VIDEO prompt
    # one spoken turn in front of a spoken turn: clips in history order, the state token loses its space
    r = merge_current_and_history([copy.deepcopy(H_AUDIO)], {"prompt": "<audio>", "multi_modal_data": {"audio": ["A9"]}}, True, True)
    assert r["prompt"] == SYS_PLAIN + "user:<audio></s>\nbot:<1>hello there.</s>\nuser:<audio></s>\nbot:"
    assert r["multi_modal_data"] == {"audio": ["A0", "A9"]}
    # history vision skipped: its token and its image go, its clip stays; the current image token moves to the start
    req = {"prompt": "<audio><image>", "multi_modal_data": {"image": ["I9"], "audio": ["A9"]}}
    r = merge_current_and_history([copy.deepcopy(H_IMAGE)], copy.deepcopy(req), True, True)
    assert r["prompt"] == SYS_VIDEO + "user:<image><audio></s>\nbot:<2>nothing</s>\nuser:<audio></s>\nbot:"
    assert r["multi_modal_data"] == {"image": ["I9"], "audio": ["A1", "A9"]}
    # ... kept: both images, both tokens, in place
    r = merge_current_and_history([copy.deepcopy(H_IMAGE)], copy.deepcopy(req), False, False)
    assert r["prompt"] == SYS_VIDEO + "user:<image><audio></s>\nbot:<2>nothing</s>\nuser:<audio><image></s>\nbot:"
    assert r["multi_modal_data"] == {"image": ["I1", "I9"], "audio": ["A1", "A9"]}
    # the image-token move strips a character SET, as the reference's lstrip does: "sunny" loses "su"
    r = merge_current_and_history([{"prompt": "sunny", "response": "ok"}], {"prompt": "<image>", "multi_modal_data": {"image": ["I"]}},
                                  True, True)
    assert r["prompt"] == SYS_VIDEO + "user:<image>" + "nny</s>\nbot:ok</s>\nuser:</s>\nbot:"
    with pytest.raises(AssertionError):
        merge_current_and_history([{"prompt": "no answer"}], {"prompt": "x"})


def test_valid_rows_of_a_clip_are_audio_feature_size():
    """the serving splice keeps the rows the encoder's mask marks valid: (arange(T2) < klen)[0::2] with klen from the clip's frames
    at ANY padded length — the count expanded_token_ids assumes (serving.audio_feature_size)."""
    from vita_amd.serving import audio_feature_size
    for L in list(range(8, 400)) + [640, 998, 1500, 3000]:
        for T in (L, L + 1, L + 37, 3000):
            klen = len(range(T)[:L][2::2][2::2])
            assert (klen + 1) // 2 == audio_feature_size(L), (L, T)


# ---- the turn protocol on scripted engines ---------------------------------------------------------------------------------------
class RecordingLLM:
    """generate_stream yields the request's script as cumulative text and records the inputs it was handed."""
    seen = []
    tokenizer = None

    def generate_stream(self, inputs, sampling_params=None, request_id=None, should_stop=None):
        RecordingLLM.seen.append(copy.deepcopy(inputs))
        text = ""
        for chunk in inputs["script"]:
            time.sleep(0.002)
            text += chunk
            yield SimpleNamespace(outputs=[SimpleNamespace(text=text, token_ids=[])])


class _CharTokenizer:
    bos_token_id = 1

    def __call__(self, text):
        return SimpleNamespace(input_ids=[1] + [ord(c) for c in text])


class TokenizingLLM(RecordingLLM):
    tokenizer = _CharTokenizer()
    image_token_index, audio_token_index = 51000, 51001


class _Val:
    value = -1


def _setup(llm_cls, **mode):
    import queue
    ev = threading.Event
    RecordingLLM.seen = []
    sh = SimpleNamespace(inputs=queue.Queue(), outputs=queue.Queue(), stats=queue.Queue(), history=[], shutdown=ev(),
                         lock=threading.Lock(), interrupt=_Val(), ready=[ev(), ev()], stop=[ev(), ev()], start=[ev(), ev()])
    sh.start[0].set()
    th = []
    for i in range(2):
        kw = dict(inputs_queue=sh.inputs, outputs_queue=sh.outputs, stop_event=sh.stop[i], other_stop_event=sh.stop[1 - i],
                  worker_ready=sh.ready[i], wait_workers_ready=sh.ready, start_event=sh.start[i],
                  other_start_event=sh.start[1 - i], start_event_lock=sh.lock, interrupt_signal=sh.interrupt,
                  global_history=sh.history, shutdown_event=sh.shutdown, stats_queue=sh.stats, poll_s=0.001, **mode)
        t = threading.Thread(target=duplex.worker_loop, args=(i, llm_cls, None), kwargs=kw, daemon=True)
        t.start()
        th.append(t)
    return sh, th


def _turn(sh, request, timeout=5.0):
    sh.inputs.put(request)
    t0 = time.time()
    while time.time() - t0 < timeout:
        try:
            return sh.stats.get(timeout=0.05)
        except Exception:
            pass
    raise AssertionError("the turn was not answered (did the worker start?)")


def _spoken(i, clip, script):
    return {"prompt": "<audio>", "multi_modal_data": {"audio": [clip]}, "request_id": i, "script": script}


@pytest.mark.timeout(60)
def test_second_turn_receives_the_merged_prompt_and_both_clips():
    sh, th = _setup(RecordingLLM, conversation=True, history_turns=1)
    try:
        s0 = _turn(sh, _spoken(0, "clip0", ["<1> ", "first", " answer", "."]))
        s1 = _turn(sh, _spoken(1, "clip1", ["<1> ", "second", "."]))
        assert [s0["id"], s1["id"]] == [0, 1] and not s0["error"] and not s1["error"]
        a, b = RecordingLLM.seen
        assert a["prompt"] == SYS_PLAIN + "user:<audio></s>\nbot:" and a["multi_modal_data"] == {"audio": ["clip0"]}
        assert b["prompt"] == SYS_PLAIN + "user:<audio></s>\nbot:<1>first answer.</s>\nuser:<audio></s>\nbot:"
        assert b["multi_modal_data"] == {"audio": ["clip0", "clip1"]}            # [history clip, current clip]
        assert "prompt_token_ids" not in b                                        # this engine has no tokenizer
        # the history keeps the UNMERGED request: prompt, modal data, response
        assert sh.history == [{"prompt": "<audio>", "multi_modal_data": {"audio": ["clip0"]}, "response": "<1> first answer."},
                              {"prompt": "<audio>", "multi_modal_data": {"audio": ["clip1"]}, "response": "<1> second."}]
    finally:
        sh.shutdown.set()
        [t.join(timeout=2) for t in th]


@pytest.mark.timeout(60)
def test_noise_leaves_no_history_and_history_turns_bounds_the_memory():
    sh, th = _setup(RecordingLLM, conversation=True, history_turns=1)
    try:
        _turn(sh, _spoken(0, "clip0", ["<1> ", "one", "."]))
        noise = _turn(sh, _spoken(1, "clipN", ["<2>", " ignored", "."]))
        assert noise["negative"] and [h["multi_modal_data"]["audio"] for h in sh.history] == [["clip0"]]
        _turn(sh, _spoken(2, "clip2", ["<1> ", "two", "."]))
        _turn(sh, _spoken(3, "clip3", ["<1> ", "three", "."]))
        seen = RecordingLLM.seen
        assert seen[1]["multi_modal_data"] == {"audio": ["clip0", "clipN"]}      # the noise turn itself was asked with memory
        assert seen[2]["multi_modal_data"] == {"audio": ["clip0", "clip2"]}      # ... and left none: turn 2 still sees turn 0
        assert seen[2]["prompt"] == SYS_PLAIN + "user:<audio></s>\nbot:<1>one.</s>\nuser:<audio></s>\nbot:"
        assert seen[3]["multi_modal_data"] == {"audio": ["clip2", "clip3"]}      # history_turns = 1: the third answer sees only the second
        assert seen[3]["prompt"] == SYS_PLAIN + "user:<audio></s>\nbot:<1>two.</s>\nuser:<audio></s>\nbot:"
    finally:
        sh.shutdown.set()
        [t.join(timeout=2) for t in th]


@pytest.mark.timeout(60)
def test_two_history_turns_and_an_image_turn():
    sh, th = _setup(RecordingLLM, conversation=True, history_turns=2)
    try:
        _turn(sh, _spoken(0, "clip0", ["<1> ", "one", "."]))
        _turn(sh, {"prompt": "<image><audio>", "multi_modal_data": {"image": ["img1"], "audio": ["clip1"]}, "request_id": 1,
                   "script": ["<1> ", "a", " cat", "."]})
        _turn(sh, _spoken(2, "clip2", ["<1> ", "three", "."]))
        last = RecordingLLM.seen[2]
        assert last["multi_modal_data"] == {"audio": ["clip0", "clip1", "clip2"]}          # the history image is skipped
        assert last["prompt"] == (SYS_PLAIN + "user:<audio></s>\nbot:<1>one.</s>\nuser:<audio></s>\nbot:<1>a cat.</s>\n"
                                  "user:<audio></s>\nbot:")
        mid = RecordingLLM.seen[1]
        assert mid["prompt"] == SYS_VIDEO + "user:<image><audio></s>\nbot:<1>one.</s>\nuser:<audio></s>\nbot:"   # image token first
        assert mid["multi_modal_data"] == {"image": ["img1"], "audio": ["clip0", "clip1"]}
    finally:
        sh.shutdown.set()
        [t.join(timeout=2) for t in th]


@pytest.mark.timeout(60)
def test_merged_prompt_is_tokenised_with_the_engines_placeholder_ids():
    sh, th = _setup(TokenizingLLM, conversation=True)
    try:
        _turn(sh, _spoken(0, "clip0", ["<1> ", "ok", "."]))
        _turn(sh, {"prompt": "<image><audio>", "multi_modal_data": {"image": ["img"], "audio": ["clip1"]}, "request_id": 1,
                   "script": ["<1> ", "fine", "."]})
        ids = RecordingLLM.seen[1]["prompt_token_ids"]
        text = RecordingLLM.seen[1]["prompt"]
        assert ids[0] == 1 and ids.count(1) == 1                                  # one BOS
        assert [t for t in ids if t >= 51000] == [51000, 51001, 51001]            # image first, then history clip, current clip
        assert "".join(chr(t) for t in ids[1:] if t < 51000) == text.replace("<image>", "").replace("<audio>", "")
    finally:
        sh.shutdown.set()
        [t.join(timeout=2) for t in th]


@pytest.mark.timeout(60)
def test_conversation_off_hands_the_engine_what_was_submitted():
    sh, th = _setup(RecordingLLM)
    try:
        r0, r1 = _spoken(0, "clip0", ["<1> ", "one", "."]), _spoken(1, "clip1", ["<1> ", "two", "."])
        _turn(sh, copy.deepcopy(r0))
        _turn(sh, copy.deepcopy(r1))
        assert RecordingLLM.seen == [r0, r1]
        assert sh.history == [{"prompt": "<audio>", "response": "<1> one."}, {"prompt": "<audio>", "response": "<1> two."}]
    finally:
        sh.shutdown.set()
        [t.join(timeout=2) for t in th]
