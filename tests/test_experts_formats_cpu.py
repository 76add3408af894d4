"""The argument checks that bf16, int8 and MXFP4 experts share, without a GPU: the per-operator MoE decode entries refuse null
pointers and bad widths before any device call, and vh_mixtral_create refuses bf16 layers with a missing expert weight."""
import ctypes as C

import pytest

FAKE = 0x1000                                                # never dereferenced: every refusal comes before device work

# entry -> its argument names in order (vita_hip.h); delta and x_out are optional, the stream may be null
_HEAD = ["x", "delta", "norm_w", "eps", "Wg"]
_TAIL = ["E", "I", "H", "x_out", "y", "route", "hbuf", "stream"]
ENTRIES = {
    "vh_moe_decode": _HEAD + ["W1", "W3", "W2"] + _TAIL,
    "vh_moe_decode_i8": _HEAD + ["W1", "s1", "W3", "s3", "W2", "s2"] + _TAIL,
    "vh_moe_decode_mxfp4": _HEAD + ["W1", "s1", "W3", "s3", "W2", "s2"] + _TAIL,
}
OPTIONAL = ("delta", "x_out", "stream")


def _lib():
    from vita_amd import _lib
    return _lib.load()                                       # no GPU needed; an unbuilt library or a missing symbol fails the test


def _call(lib, entry, **kw):
    vals = {"eps": 1e-5, "E": 4, "I": 256, "H": 128, "stream": None}
    vals.update(kw)
    rc = getattr(lib, entry)(*[vals.get(name, FAKE) for name in ENTRIES[entry]])
    return rc, lib.vh_last_error()


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_moe_decode_argument_checks(entry):
    lib = _lib()
    name = entry.encode()
    for arg in ENTRIES[entry]:
        if arg in OPTIONAL or arg in ("eps", "E", "I", "H"):
            continue
        rc, msg = _call(lib, entry, **{arg: None})           # every required pointer, one at a time
        assert rc == -2 and msg.startswith(name + b":") and b"null" in msg, (arg, rc, msg)
    for kw in ({"H": 96}, {"I": 96}, {"H": 14400}, {"I": 14400}):   # not a multiple of 64; a multiple of 64 above 14336
        rc, msg = _call(lib, entry, **kw)
        assert rc == -1 and msg.startswith(name + b":") and b"multiples of 64" in msg, (kw, rc, msg)


def _bf16_layers():
    from vita_amd._lib import MixtralCfg, MixtralLayer
    c = MixtralCfg()
    c.hidden, c.n_layers, c.n_q_heads, c.n_kv_heads, c.head_dim = 128, 2, 4, 2, 128
    c.inter, c.n_experts, c.top_k, c.vocab, c.rms_eps = 256, 4, 2, 512, 1e-5
    c.max_ctx, c.max_prefill, c.max_new = 128, 64, 16
    layers = (MixtralLayer * 2)()
    for L in layers:
        for f, _ in MixtralLayer._fields_:
            setattr(L, f, FAKE)
    return c, layers


def test_create_bf16_refuses_a_null_expert_weight():
    lib = _lib()
    c, layers = _bf16_layers()
    args = (FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 30)
    for field in ("w2", "w1", "w3"):
        setattr(layers[1], field, None)
        assert not lib.vh_mixtral_create(C.byref(c), layers, *args), field
        msg = lib.vh_last_error()
        assert msg.startswith(b"vh_mixtral_create:") and b"layers[1]" in msg and b"null" in msg, (field, msg)
        setattr(layers[1], field, FAKE)
    m = lib.vh_mixtral_create(C.byref(c), layers, *args)      # all three set: an engine (creation touches no device memory)
    assert m, lib.vh_last_error()
    lib.vh_mixtral_destroy(m)
