"""ORACLE (test infrastructure): records what the REFERENCE'S OWN modules and functions compute on the seeded inputs of the
pin tests tests/test_oracle_pin.py test_live_* and tests/test_host_logic.py test_audio_side_files_* /
test_video_front_end_*, so those tests need nothing outside the repository.
The seeded inputs are made by the functions below, which the tests call too.  Writes tests/golden/reference_pins.npz:

  live_vit, live_whale              InternViT tower and Whale encoder + adapter of the reference on live_inputs()
  pad_embeds, pad_mask              the reference Whale's inputs_embeds and attention_mask of pad_inputs(): two clips of
                                    different lengths in ONE batch
  cmvn_{json,kaldi}_{mean,istd}     whale/cmvn.py load_cmvn on the two side files of cmvn_files()
  video_{i}, video_n_{i}            video_audio_demo.py _get_rawvideo_dec on the synthetic containers of video_cases()

    python -m oracle.make_golden_pins
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "reference_pins.npz")

LIVE_SEEDS = (11, 12)
PAD_SEEDS, PAD_T, PAD_LENS = (13, 14), 140, [140, 97]
# (frames, fps, kwargs of the frame sampler); the frames are drawn one case after another from default_rng(0)
VIDEO_CASES = ((70, 5.0, {}), (9, 3.0, {}), (400, 10.0, {}), (120, 4.0, {"s": 3, "e": 11}))
VIDEO_PROC_SIZE = 56


def live_inputs():
    rng = np.random.default_rng(LIVE_SEEDS[1])
    pix = rng.standard_normal((1, 3, 56, 56)).astype(np.float32)
    feats = (rng.standard_normal((77, 80)) * 2 + 10).astype(np.float32)
    return pix, feats


def pad_inputs():
    rng = np.random.default_rng(PAD_SEEDS[1])
    return (rng.standard_normal((2, PAD_T, 80)) * 3 + 12).astype(np.float32)


def cmvn_files(d):
    """writes the JSON and the Kaldi-text form of one set of CMVN statistics into directory d: (paths, mean, inverse std)."""
    rng = np.random.default_rng(4)
    n, dim = 12345.0, 80
    s1 = rng.standard_normal(dim) * 40 * n
    s2 = (rng.random(dim) * 30 + (s1 / n) ** 2) * n
    pj, pk = os.path.join(d, "cmvn.json"), os.path.join(d, "global_cmvn")
    with open(pj, "w") as f:
        f.write(json.dumps({"mean_stat": s1.tolist(), "var_stat": s2.tolist(), "frame_num": n}))
    with open(pk, "w") as f:
        f.write("[\n " + " ".join(repr(float(x)) for x in s1) + f" {n!r}\n " + " ".join(repr(float(x)) for x in s2) + " 0 ]\n")
    mean = s1 / n
    istd = 1.0 / np.sqrt(np.maximum(s2 / n - mean * mean, 1e-20))
    return {"json": (pj, True), "kaldi": (pk, False)}, mean, istd


def video_cases(d):
    """writes the synthetic frame containers (read by compat/decord) into directory d: [(path, kwargs)]."""
    rng = np.random.default_rng(0)
    out = []
    for T, fps, kw in VIDEO_CASES:
        path = os.path.join(d, f"v{T}.npz")
        np.savez(path, frames=rng.integers(0, 255, size=(T, 40, 60, 3), dtype=np.uint8), fps=fps)
        out.append((path, kw))
    return out


def main():
    import importlib.util
    import logging
    import tempfile

    import torch
    from oracle import ref_harness as rh
    from vita_amd.checkpoint import synth_state_dict
    from vita_amd.config import VitaConfig
    assert rh.available(), "needs the reference tree"
    rh.install()
    g = {}
    cfg = VitaConfig.tiny()

    sd = synth_state_dict(cfg, seed=LIVE_SEEDS[0])
    pix, feats = live_inputs()
    with torch.no_grad():
        g["live_vit"] = rh.build_internvit(cfg, sd)(torch.from_numpy(pix)).numpy()
        g["live_whale"] = rh.build_whale(cfg, sd)(torch.from_numpy(feats)[None], torch.tensor([77]))["inputs_embeds"][0].numpy()

    sd = synth_state_dict(cfg, seed=PAD_SEEDS[0])
    feats = pad_inputs()
    with torch.no_grad():
        ref = rh.build_whale(cfg, sd)(torch.from_numpy(feats), torch.tensor(PAD_LENS))
    g["pad_embeds"], g["pad_mask"] = ref["inputs_embeds"].numpy(), ref["attention_mask"].numpy().astype(bool)

    from vita.model.multimodal_encoder.whale import cmvn as rc
    rc.logging, rc.sys = logging, sys          # the reference's kaldi loader uses names it never imports
    with tempfile.TemporaryDirectory() as d:
        files, _, _ = cmvn_files(d)
        for kind, (path, is_json) in files.items():
            g[f"cmvn_{kind}_mean"], g[f"cmvn_{kind}_istd"] = rc.load_cmvn(path, is_json)

    # the demo script's video reader, imported with compat/ serving `vita.*` and `decord` (instead of the harness stubs)
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    for k in [k for k in sys.modules if k in ("vita", "decord") or k.startswith(("vita.", "decord."))]:
        sys.modules.pop(k)
    spec = importlib.util.spec_from_file_location("ref_video_audio_demo", os.path.join(rh.REF, "video_audio_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    from vita_amd.host.image_processing import make_image_processor
    proc = make_image_processor(VIDEO_PROC_SIZE)
    with tempfile.TemporaryDirectory() as d:
        for i, (path, kw) in enumerate(video_cases(d)):
            want, n_want = demo._get_rawvideo_dec(path, proc, max_frames=16, min_frames=4, video_framerate=1,
                                                  image_aspect_ratio="pad", **kw)
            g[f"video_{i}"], g[f"video_n_{i}"] = want.numpy(), np.asarray(n_want)

    np.savez_compressed(OUT, **g)
    print("written", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
