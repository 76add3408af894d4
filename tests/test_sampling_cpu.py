"""The sampling contract's numpy restatement (tests/sampling_ref.py) against third parties: its Philox4x64-10 against
numpy.random.Philox, its top-k / top-p kept set against transformers' TopKLogitsWarper + TopPLogitsWarper; and the vh_sampling
ctypes mirror against the C header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import sampling_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 1 << 64


def numpy_block(seed, counter):
    """the four words numpy's Philox emits for block `counter` (4 uint64 words, little-endian): numpy increments its counter
    BEFORE generating, so it is set one below (with the borrow carried across words)."""
    c = sum(int(w) << (64 * j) for j, w in enumerate(counter))
    c = (c - 1) % (1 << 256)
    g = np.random.Philox(key=seed, counter=c)
    return [int(w) for w in g.random_raw(4)]


@pytest.mark.parametrize("seed", [0, 1, 12345, U64 - 1, 0x9E3779B97F4A7C15])
def test_philox_matches_numpy(seed):
    counters = [(0, 0, 0, 0), (1, 0, 0, 0), (7, 3, 0, 0), (U64 - 1, 5, 0, 0), (0, 1, 0, 0), (123456789, 987654321, 0, 0),
                (0, U64 - 1, 0, 0), (3, 4, 5, 6), (U64 - 1, U64 - 1, 0, 0)]
    for ctr in counters:
        got = ref.philox4x64(*[np.array([w], dtype=np.uint64) for w in ctr], seed, 0)
        assert [int(w[0]) for w in got] == numpy_block(seed, ctr), (seed, ctr)


def test_gumbel_words_follow_the_index():
    """G_i uses word i & 3 of block i >> 2: the vectorised restatement against one block at a time."""
    seed, draw = 77, 1234
    idx = np.arange(40)
    g = ref.gumbel(seed, draw, idx)
    for i in idx:
        x = numpy_block(seed, (i >> 2, draw, 0, 0))[i & 3]
        u = ((x >> 11) + 0.5) * 2.0 ** -53
        assert g[i] == -np.log(-np.log(u))


def test_kept_set_matches_transformers_warpers():
    torch = pytest.importorskip("torch")
    tf = pytest.importorskip("transformers")
    rng = np.random.default_rng(5)
    cases = 0
    for V in (50, 1000, 4001):
        for T in (0.01, 0.7, 1.0, 1.5):
            for top_k in (0, 1, 5, 50, V):
                for top_p in (1.0, 0.95, 0.5, 1e-6):
                    row = (rng.standard_normal(V) * 3).astype(np.float32)
                    while np.unique(row).shape[0] < V:            # tie-free rows only
                        row = (rng.standard_normal(V) * 3).astype(np.float32)
                    z = ref.scaled(row, T)
                    s = torch.from_numpy(z)[None]
                    if top_k > 0:
                        s = tf.TopKLogitsWarper(top_k=top_k)(None, s)
                    if float(np.float32(top_p)) < 1.0:
                        s = tf.TopPLogitsWarper(top_p=float(np.float32(top_p)))(None, s)
                    hf = torch.isfinite(s[0]).numpy()
                    got = ref.keep_mask(row, T, top_k, top_p)
                    assert np.array_equal(got, hf), (V, T, top_k, top_p, int(got.sum()), int(hf.sum()))
                    cases += 1
    assert cases == 3 * 4 * 5 * 4


def test_restatement_degenerate_rows():
    row = np.array([0.5, np.nan, 2.0, -np.inf, 2.0], dtype=np.float32)
    assert ref.sample(row, 0.0) == 2                              # greedy: first maximum, NaN never wins
    assert ref.sample(row, 1.0, top_k=1, seed=3) in (2, 4)          # both tied maxima kept
    assert ref.sample(np.full(7, np.nan, dtype=np.float32), 1.0, seed=1) == 0
    assert ref.sample(np.full(7, -np.inf, dtype=np.float32), 0.8, top_p=0.5, seed=1) == 0
    p = ref.filtered_softmax(np.log(np.array([0.5, 0.25, 0.125, 0.125], dtype=np.float32)), 1.0, top_p=0.7)
    assert np.count_nonzero(p) == 2                                 # mass above: 0 and 0.5 < 0.7, 0.75 is not
    p = ref.filtered_softmax(np.log(np.array([0.5, 0.125, 0.25, 0.125], dtype=np.float32)), 1.0, top_p=0.8)
    assert np.count_nonzero(p) == 4                                 # the tied 0.125s enter together (mass above them 0.75)


def test_sampling_struct_matches_the_header(tmp_path):
    from vita_amd import _lib
    cls = _lib.Sampling
    lines = ['printf("%zu", sizeof(vh_sampling));'] + [f'printf(" %zu", offsetof(vh_sampling, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vita_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, *offs = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert ctypes.sizeof(cls) == int(size)
    assert [getattr(cls, f).offset for f, _ in cls._fields_] == [int(o) for o in offs]
