"""numpy restatement of the int8 expert mode and the oracle helpers its tests use (oracle/ stays as it is).

    s[r]   = max_k |w[r,k]| / 127                              (fp32, IEEE division)
    q[r,k] = 0 if s[r] == 0 else clamp(rint(w[r,k] / s[r]), -127, 127)   (fp32 IEEE division, ties to even)
    w'     = q * s                                             (the model the engine computes)

w1 / w3 ([E][I][H]) are quantised per row of I, w2 ([E][H][I]) per row of H over the FULL I columns."""
import contextlib

import numpy as np

F32 = np.float32


def quant_rows(w):
    """w: [..., cols] values (bf16 values as fp32) -> (q int8 [..., cols], s fp32 [...])."""
    w = np.asarray(w, F32)
    s = (np.abs(w).max(axis=-1) / F32(127)).astype(F32)
    safe = np.where(s == 0, F32(1), s).astype(F32)
    q = np.clip(np.rint(w / safe[..., None]), -127, 127).astype(np.int8)
    q[s == 0] = 0
    return q, s


def dequant(q, s):
    return (q.astype(F32) * np.asarray(s, F32)[..., None]).astype(F32)


def wprime(w):
    return dequant(*quant_rows(w))


def is_expert_key(k):
    return ".block_sparse_moe.experts." in k and k.rsplit(".", 2)[-2] in ("w1", "w2", "w3")


def dequant_state_dict(sd):
    """reference-named state dict with every expert weight replaced by w' (fp32); everything else as it is."""
    return {k: (wprime(v) if is_expert_key(k) else v) for k, v in sd.items()}


@contextlib.contextmanager
def streamed_experts_wprime():
    """oracle.stream.LayerBuffers.load with w1 / w3 / w2 replaced by w' while the context is open (the streamed oracle of the
    released geometry regenerates the bf16 weights layer by layer; this quantises them as the engine does)."""
    from oracle import stream
    orig = stream.LayerBuffers.load

    def load(self, *a, **k):
        r = orig(self, *a, **k)
        for nm in ("w1", "w3", "w2"):
            for e in range(r[nm].shape[0]):          # in place, one expert at a time (the buffers are refilled per layer)
                r[nm][e] = wprime(r[nm][e])
        return r
    stream.LayerBuffers.load = load
    try:
        yield
    finally:
        stream.LayerBuffers.load = orig
