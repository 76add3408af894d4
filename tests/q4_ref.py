"""numpy restatement of the MXFP4 expert mode and the oracle helpers its tests use (oracle/ stays as it is).

Blocks of 32 consecutive elements along K (the last, contiguous dimension); K % 32 == 0.

    amax = max |w| over the block
    se   = max(floor(log2(amax)) - 2, -125)        floor(log2) from the exponent field (exact); a zero block: se = 0
    X    = 2^se ; the stored E8M0 byte is se + 127 (a zero block stores 127)
    v    = w / X (exact) ; |v| saturates at 6 and rounds to the nearest of 0, .5, 1, 1.5, 2, 3, 4, 6, ties to the even code
    code = sign << 3 | index, the sign bit only for a non-zero magnitude (no -0; readers take code 8 as 0)
    w'   = e2m1(code) * 2^(byte - 127)             (a bf16 number: the model the engine computes)

codes uint8 [..., K / 2]: element k in byte k >> 1, low nibble for even k.  scales uint8 [..., K / 32]."""
import contextlib

import numpy as np

F32 = np.float32
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], F32)
# |v| < MID[i] (or == MID[i] with the lower code even) stays at index i: the midpoints between neighbouring magnitudes
_MID = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], F32)


def block_exponent(amax):
    """se of blocks with largest magnitude amax (fp32 array): max(floor(log2(amax)) - 2, -125), 0 for amax == 0."""
    amax = np.ascontiguousarray(amax, F32)
    ef = ((amax.view(np.uint32) >> 23) & 0xFF).astype(np.int32) - 127      # bf16 values: never fp32 denormals unless 0 < amax < 2^-126
    m = amax.view(np.uint32) & 0x7FFFFF
    den = (ef == -127) & (m != 0)                                          # fp32 denormal: floor(log2) < -126, the clamp decides
    se = np.maximum(ef - 2, -125)
    se = np.where(den, -125, se)
    return np.where(amax == 0, 0, se).astype(np.int32)


def quant_codes(w):
    """w [..., K] (bf16 values as fp32, finite) -> (code uint8 [..., K] one code per element, byte uint8 [..., K / 32])."""
    w = np.asarray(w, F32)
    K = w.shape[-1]
    if K % 32:
        raise ValueError("K must be a multiple of 32")
    if not np.isfinite(w).all():
        raise ValueError("non-finite weight")
    b = w.reshape(w.shape[:-1] + (K // 32, 32))
    se = block_exponent(np.abs(b).max(axis=-1))
    X = np.ldexp(F32(1), se).astype(F32)
    v = np.minimum(np.abs(b) / X[..., None], F32(6)).astype(F32)
    idx = np.zeros(v.shape, np.uint8)
    for i, mid in enumerate(_MID):                                         # ties to the even code: up from an odd index only
        idx += ((v > mid) | ((v == mid) & (i % 2 == 1))).astype(np.uint8)
    sign = ((b < 0) & (idx != 0)).astype(np.uint8)
    code = (sign << 3 | idx).astype(np.uint8).reshape(w.shape)
    return code, (se + 127).astype(np.uint8)


def pack(code):
    """one code per element [..., K] -> packed bytes [..., K / 2] (low nibble: the even element)."""
    return (code[..., 0::2] | (code[..., 1::2] << 4)).astype(np.uint8)


def unpack(codes):
    out = np.empty(codes.shape[:-1] + (codes.shape[-1] * 2,), np.uint8)
    out[..., 0::2] = codes & 15
    out[..., 1::2] = codes >> 4
    return out


def quant(w):
    """w [..., K] -> (codes uint8 [..., K / 2] packed, scales uint8 [..., K / 32]): the canonical layout."""
    code, byte = quant_codes(w)
    return pack(code), byte


def dequant(codes, scales):
    """packed codes [..., K / 2], scale bytes [..., K / 32] -> w' fp32 [..., K]."""
    c = unpack(np.asarray(codes, np.uint8))
    mag = E2M1[c & 7] * np.where(c & 8, F32(-1), F32(1)).astype(F32)
    X = np.ldexp(F32(1), np.asarray(scales, np.uint8).astype(np.int32) - 127).astype(F32)
    return (mag.reshape(c.shape[:-1] + (-1, 32)) * X[..., None]).reshape(c.shape).astype(F32)


def _wprime_blocks(b):
    X = np.ldexp(F32(1), block_exponent(np.abs(b).max(axis=1))).astype(F32)[:, None]
    v = np.abs(b)
    v /= X
    np.minimum(v, F32(6), out=v)
    step = (F32(0.5) * (F32(1) + (v >= 2) + F32(2) * (v >= 4))).astype(F32)
    v /= step
    np.rint(v, out=v)
    v *= step
    v *= X
    return np.copysign(v, b)


def wprime(w, chunk=8192):
    """w' of w [..., K] without materialising the codes: the same values as dequant(*quant(w)) (tests/test_experts_mxfp4_cpu.py
    compares them) in a few passes over cache-sized runs of `chunk` blocks, for the streamed oracle of the released geometry.  The
    e2m1 grid has step .5 below 2, 1 below 4 and 2 above, and np.rint's ties-to-even on v / step picks the even CODE on every tie
    (the code's parity is v / step's)."""
    w = np.asarray(w, F32)
    b = w.reshape(-1, 32)
    out = np.empty_like(b)
    for i in range(0, b.shape[0], chunk):
        out[i:i + chunk] = _wprime_blocks(b[i:i + chunk])
    return out.reshape(w.shape)


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
