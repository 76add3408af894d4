"""GPU parity of every generic C-ABI operator against plain numpy (the per-kernel oracle):
fp32 references on the same bf16-rounded weights.  Tolerances: the split-bf16 GEMM carries the
activation to 2^-17, so |err| <= ~2e-5 * sum|a*w| in the worst case; stated per test."""
import numpy as np
import pytest
import torch

from tests.util import assert_close, to_np
from vita_amd.checkpoint import round_bf16

pytestmark = pytest.mark.gpu

# plain / causal attention runs on bf16 x 3 MFMAs (vh_attn.hip k_attn_x3): every q.k and p.v product is exact to ~2^-17 of its
# magnitude, as in the exact-mode GEMMs; at N(0,1) operands and d <= 128 that is < 1e-4 on the output
ATTN_X3_ATOL = 1e-4


def _w(rng, *shape, std=0.05):
    return round_bf16(rng.standard_normal(shape, dtype=np.float32) * std)


def _dev(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dtype)


def gelu(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


ACTS = {None: lambda x: x, "gelu": gelu, "relu": lambda x: np.maximum(x, 0), "silu": lambda x: x / (1 + np.exp(-x))}


# ---------------------------------------------------------------------------------------------
def test_mfma_layout_probe(dev):
    """A = I-like pattern with an ASYMMETRIC W catches row/col swaps of the MFMA fragment maps."""
    from vita_amd import ops
    M, N, K = 64, 128, 64
    a = np.zeros((M, K), np.float32)
    a[np.arange(M), np.arange(M) % K] = 1.0
    w = round_bf16((np.arange(N)[:, None] * 0.5 + np.arange(K)[None, :] * 0.001953125).astype(np.float32))
    got = to_np(ops.gemm(_dev(a, dev), _dev(w, dev, torch.bfloat16)))
    assert_close("mfma_layout", got, a.astype(np.float64) @ w.T.astype(np.float64), atol=1e-4)


@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (7, 100, 128), (64, 128, 64), (130, 257, 192), (450, 6144, 4096),
                                   (1025, 3072, 1024)])
def test_gemm_plain(dev, M, N, K):
    from vita_amd import ops
    rng = np.random.default_rng(M * 7 + N)
    a = rng.standard_normal((M, K), dtype=np.float32)
    w = _w(rng, N, K)
    got = to_np(ops.gemm(_dev(a, dev), _dev(w, dev, torch.bfloat16)))
    ref = a.astype(np.float64) @ w.T.astype(np.float64)
    assert_close(f"gemm {M}x{N}x{K}", got, ref, atol=2e-5 * np.sqrt(K), rtol=2e-5)


@pytest.mark.parametrize("act", [None, "gelu", "relu", "silu"])
def test_gemm_epilogue(dev, act):
    from vita_amd import ops
    rng = np.random.default_rng(3)
    M, N, K = 77, 200, 128
    a = rng.standard_normal((M, K), dtype=np.float32)
    w = _w(rng, N, K)
    bias, scale = _w(rng, N, std=0.5), _w(rng, N, std=1.0)
    resid = rng.standard_normal((M, N), dtype=np.float32)
    got = to_np(ops.gemm(_dev(a, dev), _dev(w, dev, torch.bfloat16), bias=_dev(bias, dev), act=act,
                         scale=_dev(scale, dev), resid=_dev(resid, dev)))
    ref = ACTS[act](a.astype(np.float64) @ w.T + bias) * scale + resid
    assert_close(f"gemm epilogue {act}", got, ref, atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("ksplit", [0, 1, 3, 8])
def test_gemm_split_k(dev, ksplit):
    """split-K (partial slabs + reducing kernel with the whole epilogue) against the fp64 reference, on the encoder shape
    that leaves half the chip idle unsplit (M = 1025, N = 1024, K = 4096: 136 blocks), in-place residual included."""
    from vita_amd import ops
    rng = np.random.default_rng(40)
    M, N, K = 1025, 1024, 4096
    a = rng.standard_normal((M, K), dtype=np.float32)
    w = _w(rng, N, K)
    bias, scale = _w(rng, N, std=0.5), _w(rng, N, std=1.0)
    x = rng.standard_normal((M, N), dtype=np.float32)
    xd = _dev(x, dev)
    ops.gemm(_dev(a, dev), _dev(w, dev, torch.bfloat16), bias=_dev(bias, dev), act="gelu", scale=_dev(scale, dev),
             resid=xd, out=xd, ksplit=ksplit)
    ref = ACTS["gelu"](a.astype(np.float64) @ w.T + bias) * scale + x
    assert_close(f"gemm split-K {ksplit}", to_np(xd), ref, atol=2e-5 * np.sqrt(K), rtol=2e-5)
    # a small-K launch never splits below 4 K-tiles per block, a ragged N (not % 4) never splits
    a2 = rng.standard_normal((70, 192), dtype=np.float32)
    w2 = _w(rng, 130, 192)
    got = to_np(ops.gemm(_dev(a2, dev), _dev(w2, dev, torch.bfloat16), ksplit=ksplit))
    assert_close("ragged", got, a2.astype(np.float64) @ w2.T.astype(np.float64), atol=1e-4, rtol=2e-5)


@pytest.mark.parametrize("M,N,K,ksplit,with_bias", [(1025, 1024, 1024, 0, True), (249, 1024, 4096, 0, True), (249, 1024, 1024, 1, False),
                                                   (5125, 1024, 1024, 0, True), (33, 256, 128, 0, False)])
def test_gemm_with_layernorm(dev, M, N, K, ksplit, with_bias):
    """vh_gemm_ln: the Linear (+ bias, layer scale, in-place residual) and the LayerNorm of its output in one call — through
    the split-K reducer that norms whole rows (one tile / one clip), and through the norm launch that follows an unsplit
    GEMM (5 tiles; ksplit = 1; tiny K) — against the fp64 composition (modeling_intern_vit.py:245-253)."""
    from vita_amd import ops
    rng = np.random.default_rng(M + N)
    a = rng.standard_normal((M, K), dtype=np.float32)
    w = _w(rng, N, K)
    bias, scale = _w(rng, N, std=0.5), _w(rng, N, std=1.0)
    lw, lb = 1.0 + _w(rng, N, std=0.2), _w(rng, N, std=0.3)
    x = rng.standard_normal((M, N), dtype=np.float32)
    xd = _dev(x, dev)
    out, h = ops.gemm(_dev(a, dev), _dev(w, dev, torch.bfloat16), bias=_dev(bias, dev), scale=_dev(scale, dev), resid=xd, out=xd,
                      ksplit=ksplit, ln=(_dev(lw, dev), _dev(lb, dev) if with_bias else None, 1e-6))
    assert out.data_ptr() == xd.data_ptr()
    ref = (a.astype(np.float64) @ w.T + bias) * scale + x
    mu, var = ref.mean(-1, keepdims=True), ref.var(-1, keepdims=True)
    ref_h = (ref - mu) / np.sqrt(var + 1e-6) * lw + (lb if with_bias else 0.0)
    assert_close("gemm_ln: C", to_np(xd), ref, atol=2e-5 * np.sqrt(K), rtol=2e-5)
    assert_close("gemm_ln: LayerNorm(C)", to_np(h), ref_h, atol=5e-5 * np.sqrt(K), rtol=2e-5)


def test_gemm_inplace_residual(dev):
    """out aliases resid (the x += proj(...) pattern)."""
    from vita_amd import ops
    rng = np.random.default_rng(4)
    M, N, K = 90, 128, 64
    a = rng.standard_normal((M, K), dtype=np.float32)
    w = _w(rng, N, K)
    x = rng.standard_normal((M, N), dtype=np.float32)
    xd = _dev(x, dev)
    ops.gemm(_dev(a, dev), _dev(w, dev, torch.bfloat16), resid=xd, out=xd)
    assert_close("gemm inplace resid", to_np(xd), x + a.astype(np.float64) @ w.T, atol=1e-4)


def test_gemm_segments_conv(dev):
    """conv2d 3x3 stride 2 over a channels-last map expressed as row-offset segments
    (whale subsampling conv2: subsampling.py:28-43)."""
    from vita_amd import ops
    rng = np.random.default_rng(5)
    T1, F1, Cin, Cout = 13, 9, 64, 96
    x = rng.standard_normal((T1, F1, Cin), dtype=np.float32)
    wt = _w(rng, Cout, Cin, 3, 3)  # torch layout [Cout, Cin, kh, kw]
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    ref = np.zeros((T2, F2, Cout))
    for t in range(T2):
        for f in range(F2):
            patch = x[2 * t:2 * t + 3, 2 * f:2 * f + 3, :]  # [kh, kw, Cin]
            ref[t, f] = np.einsum("hwc,ochw->o", patch.astype(np.float64), wt.astype(np.float64))
    wp = np.ascontiguousarray(wt.transpose(0, 2, 3, 1).reshape(Cout, 9 * Cin))  # [Cout, (kh,kw,cin)]
    rowidx = np.array([(2 * t) * F1 + 2 * f for t in range(T2) for f in range(F2)], np.int32)
    segrow = [kh * F1 + kw for kh in range(3) for kw in range(3)]
    got = to_np(ops.gemm(_dev(x.reshape(T1 * F1, Cin), dev), _dev(wp, dev, torch.bfloat16),
                         a_rowidx=_dev(rowidx, dev, torch.int32), segrow=segrow, seglen=Cin))
    assert_close("gemm conv segments", got, ref.reshape(T2 * F2, Cout), atol=1e-4)


def test_gemm_segments_zero_pad(dev):
    """conv1d k=5 s=2 with right zero padding via out-of-range rows (whale adapter.py:107-127)."""
    from vita_amd import ops
    rng = np.random.default_rng(6)
    T, Cin, Cout, k = 11, 64, 80, 5
    x = rng.standard_normal((T, Cin), dtype=np.float32)
    wt = _w(rng, Cout, Cin, k)
    xp = np.concatenate([x, np.zeros((k - 1, Cin), np.float32)])
    To = (T + k - 1 - k) // 2 + 1
    ref = np.stack([np.einsum("kc,ock->o", xp[2 * t:2 * t + k].astype(np.float64), wt.astype(np.float64))
                    for t in range(To)])
    wp = np.ascontiguousarray(wt.transpose(0, 2, 1).reshape(Cout, k * Cin))
    rowidx = (2 * np.arange(To)).astype(np.int32)
    got = to_np(ops.gemm(_dev(x, dev), _dev(wp, dev, torch.bfloat16), a_rowidx=_dev(rowidx, dev, torch.int32),
                         segrow=list(range(k)), seglen=Cin))  # rows >= T read as zero
    assert_close("gemm conv1d zero pad", got, ref, atol=1e-4)


def test_gemm_grouped_glu_and_scatter(dev):
    """The top-2 MoE pair: grouped gate/up GEMM with SiLU*up, then grouped down GEMM scattered to
    (token, slot) rows — HF MixtralExperts (modeling_mixtral.py:57-93)."""
    from vita_amd import ops
    rng = np.random.default_rng(7)
    S, H, I, E = 150, 128, 192, 4
    x = rng.standard_normal((S, H), dtype=np.float32)
    w1, w3, w2 = _w(rng, E, I, H), _w(rng, E, I, H), _w(rng, E, H, I)
    ids = np.stack([rng.permutation(E)[:2] for _ in range(S)]).astype(np.int32)
    ids[:10] = [[2, 0]] * 10  # skew: expert 1 may get few rows
    flat = ids.reshape(-1)
    order = np.argsort(flat, kind="stable")
    goff = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=E))]).astype(np.int32)
    stok, sslot = (order // 2).astype(np.int32), order.astype(np.int32)
    h = ops.gemm(_dev(x, dev), _dev(w1, dev, torch.bfloat16), w_up=_dev(w3, dev, torch.bfloat16),
                 a_rowidx=_dev(stok, dev, torch.int32), group_off=_dev(goff, dev, torch.int32), ngroups=E,
                 w_group_stride=I * H, m=2 * S)
    href = np.zeros((2 * S, I))
    for p, slot in enumerate(order):
        e, t = flat[slot], slot // 2
        g, u = x[t].astype(np.float64) @ w1[e].T, x[t].astype(np.float64) @ w3[e].T
        href[p] = g / (1 + np.exp(-g)) * u
    assert_close("grouped GLU", to_np(h), href, atol=2e-4)
    y = torch.zeros((2 * S, H), dtype=torch.float32, device=dev)
    ops.gemm(h, _dev(w2, dev, torch.bfloat16), group_off=_dev(goff, dev, torch.int32), ngroups=E,
             w_group_stride=H * I, c_rowidx=_dev(sslot, dev, torch.int32), out=y)
    yref = np.zeros((2 * S, H))
    hn = to_np(h).astype(np.float64)
    for p, slot in enumerate(order):
        yref[slot] = hn[p] @ w2[flat[slot]].T
    assert_close("grouped down + scatter", to_np(y), yref, atol=2e-4)


@pytest.fixture(params=[-1, 0, 1, 2], ids=["cfg-auto", "cfg-dma-ring", "cfg-regstaged", "cfg-specialised"])
def ps_cfg(request):
    """every vh_gemm_ps test runs on the default selection (by rows per group) and on each kernel form forced: 64-row tiles
    with the weights in an LDS-DMA ring, 192-row tiles with register-staged weights (all 8 waves load and multiply), and the
    12-wave form with dedicated loader waves (vh_gemm_sp.hip)."""
    from vita_amd import _lib
    _lib.tune("ps_cfg", request.param)
    yield request.param
    _lib.tune("ps_cfg", -1)


def test_gemm_ps_ksplit_slabs(dev, ps_cfg):
    """K-split down projection: partial slabs per K range add up to the unsplit product; ragged expert sizes,
    an empty expert, more experts than XCD runs."""
    from vita_amd import ops
    rng = np.random.default_rng(21)
    M, H, I, E = 200, 192, 448, 6
    h = rng.standard_normal((M, I), dtype=np.float32)
    w2 = _w(rng, E, H, I)
    cnt = np.array([70, 0, 33, 1, 80, 16])
    goff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    perm = rng.permutation(M).astype(np.int32)
    hh, hl = ops.split_planes(_dev(h, dev))
    for ks in (1, 2, 3):
        y = torch.full((ks, M, H), 7.0, dtype=torch.float32, device=dev)
        ops.gemm_ps(hh, hl, _dev(w2, dev, torch.bfloat16), group_off=_dev(goff, dev, torch.int32), ngroups=E,
                    w_group_stride=H * I, c_rowidx=_dev(perm, dev, torch.int32), out=y if ks > 1 else y[0], ksplit=ks)
        ref = np.zeros((M, H))
        for e in range(E):
            for p in range(goff[e], goff[e + 1]):
                ref[perm[p]] = h[p].astype(np.float64) @ w2[e].T
        assert_close(f"ksplit {ks}", to_np(y.sum(0)), ref, atol=2e-4)


@pytest.mark.parametrize("cnt", [[2, 0, 1, 0, 0, 2, 0, 1], [1, 1, 1, 0, 1, 1, 0, 1], [3, 2, 4, 1, 2, 1, 2, 1], [6, 0, 0, 0, 0, 0, 0, 0]])
def test_gemm_ps_device_chosen_ksplit_few_rows(dev, cnt):
    """the down projection of an iteration of a few concurrent sequences (vh_api.hip: decode_iteration): every expert holds a handful of rows,
    the kernel picks the K split itself (ksplit = -4) and reports it; the slabs it wrote add up to the unsplit product.  With one row tile per
    expert a partial round cannot be M-split, so 4 touched experts x 16 n-tiles take 4 slabs (256 tiles: the whole chip), not 2."""
    from vita_amd import ops
    rng = np.random.default_rng(sum(cnt) * 31 + cnt[0])
    E, H, I = 8, 4096, 1024
    M = int(sum(cnt))
    h = rng.standard_normal((M, I), dtype=np.float32)
    w2 = _w(rng, E, H, I)
    goff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    perm = rng.permutation(M).astype(np.int32)
    hh, hl = ops.split_planes(_dev(h, dev))
    y = torch.full((4, M, H), 7.0, dtype=torch.float32, device=dev)
    nslab = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.gemm_ps(hh, hl, _dev(w2, dev, torch.bfloat16), group_off=_dev(goff, dev, torch.int32), ngroups=E, w_group_stride=H * I,
                c_rowidx=_dev(perm, dev, torch.int32), out=y, ksplit=-4, nslab_out=nslab)
    ks = int(nslab.item())
    assert 1 <= ks <= 4
    ref = np.zeros((M, H))
    for e in range(E):
        for p in range(goff[e], goff[e + 1]):
            ref[perm[p]] = h[p].astype(np.float64) @ w2[e].T
    assert_close(f"device-chosen ksplit {ks}", to_np(y[:ks].sum(0)), ref, atol=3e-4)
    assert torch.all(y[ks:] == 7.0)                                    # slabs above the reported count are not touched
    if torch.cuda.get_device_properties(0).multi_processor_count == 256 and sum(c > 0 for c in cnt) == 4:
        assert ks == 4


def _planes_to_f32(hi, lo):
    return hi.float() + lo.float()


def test_split_planes(dev):
    from vita_amd import ops
    rng = np.random.default_rng(17)
    x = (rng.standard_normal((37, 256), dtype=np.float32) * np.exp(rng.standard_normal((37, 256)) * 3)).astype(np.float32)
    hi, lo = ops.split_planes(_dev(x, dev))
    rec = to_np(_planes_to_f32(hi, lo))
    assert np.all(np.abs(rec - x) <= np.abs(x) * 2.0 ** -16)          # two bf16 terms carry >= 16 mantissa bits
    assert np.array_equal(to_np(hi.float()), round_bf16(x))


@pytest.mark.parametrize("M,N,K,wide", [(1, 64, 64, False), (16, 128, 64, False), (138, 300, 192, False),
                                        (193, 257, 128, True), (400, 512, 4096, True), (552, 4096, 1024, False),
                                        (288, 256, 64, False), (289, 96, 128, False), (250, 512, 320, False), (33, 40, 2048, False)])
def test_gemm_ps_plain(dev, M, N, K, wide, ps_cfg):
    """pre-split skinny GEMM vs fp64 reference on the same bf16 weights: ragged M (row tiles + clamped
    rows), N tails, several 192-row m-tiles, K long enough to wrap the LDS ring many times."""
    from vita_amd import ops
    rng = np.random.default_rng(M * 7 + N)
    x = rng.standard_normal((M, K), dtype=np.float32)
    w = _w(rng, N, K)
    b = _w(rng, N)
    r = rng.standard_normal((M, N), dtype=np.float32)
    hi, lo = ops.split_planes(_dev(x, dev))
    y = ops.gemm_ps(hi, lo, _dev(w, dev, torch.bfloat16), bias=_dev(b, dev), act="gelu", resid=_dev(r, dev), wide=wide)
    ref = gelu(x.astype(np.float64) @ w.T.astype(np.float64) + b) + r
    assert_close(f"gemm_ps {M}x{N}x{K}", to_np(y), ref, atol=3e-4 if K > 1024 else 1e-4)


def test_gemm_ps_grouped_glu_and_scatter(dev, ps_cfg):
    """the MoE pair on the pre-split kernel: gather by sorted token, grouped GLU emitting split planes,
    grouped down GEMM scattered to (token, slot) rows; one expert empty, one above 192 rows."""
    from vita_amd import ops
    rng = np.random.default_rng(8)
    S, H, I, E = 330, 128, 256, 5
    x = rng.standard_normal((S, H), dtype=np.float32)
    w1, w3, w2 = _w(rng, E, I, H), _w(rng, E, I, H), _w(rng, E, H, I)
    ids = np.stack([rng.permutation(4)[:2] for _ in range(S)]).astype(np.int32)   # expert 4 never chosen
    ids[:250] = [[1, 3]] * 250                                                      # expert 1 and 3 exceed one m-tile
    flat = ids.reshape(-1)
    order = np.argsort(flat, kind="stable")
    goff = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=E))]).astype(np.int32)
    stok, sslot = (order // 2).astype(np.int32), order.astype(np.int32)
    xh, xl = ops.split_planes(_dev(x, dev))
    hh, hl = ops.gemm_ps(xh, xl, _dev(w1, dev, torch.bfloat16), w_up=_dev(w3, dev, torch.bfloat16),
                         a_rowidx=_dev(stok, dev, torch.int32), group_off=_dev(goff, dev, torch.int32), ngroups=E,
                         w_group_stride=I * H, m=2 * S, out_split=True)
    href = np.zeros((2 * S, I))
    for p, slot in enumerate(order):
        e, t = flat[slot], slot // 2
        g, u = x[t].astype(np.float64) @ w1[e].T, x[t].astype(np.float64) @ w3[e].T
        href[p] = g / (1 + np.exp(-g)) * u
    h = _planes_to_f32(hh, hl)
    assert_close("ps grouped GLU (planes)", to_np(h), href, atol=2e-4)
    y = torch.zeros((2 * S, H), dtype=torch.float32, device=dev)
    ops.gemm_ps(hh, hl, _dev(w2, dev, torch.bfloat16), group_off=_dev(goff, dev, torch.int32), ngroups=E,
                w_group_stride=H * I, c_rowidx=_dev(sslot, dev, torch.int32), out=y)
    yref = np.zeros((2 * S, H))
    hn = to_np(h).astype(np.float64)
    for p, slot in enumerate(order):
        yref[slot] = hn[p] @ w2[flat[slot]].T
    assert_close("ps grouped down + scatter", to_np(y), yref, atol=2e-4)


# ---------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, scale, mask=None, p=None, bu=None, bv=None):
    """q [H,Sq,d], k/v [Hkv,Sk,d]; mask [Sq,Sk] True = visible."""
    H, Sq, d = q.shape
    g = H // k.shape[0]
    out = np.zeros((Sq, H * d))
    for h in range(H):
        if p is None:
            s = q[h].astype(np.float64) @ k[h // g].T
        else:
            s = (q[h] + bu[h]).astype(np.float64) @ k[h // g].T + (q[h] + bv[h]).astype(np.float64) @ p[h].T
        s = s * scale
        if mask is not None:
            s = np.where(mask, s, -np.inf)
        m = np.max(s, axis=-1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        e = np.exp(s - m)
        den = e.sum(-1, keepdims=True)
        pr = np.where(den > 0, e / np.where(den > 0, den, 1), 0.0)
        out[:, h * d:(h + 1) * d] = pr @ v[h // g]
    return out


@pytest.mark.parametrize("rows,N,groups", [(16, 77, 0), (32, 77, 0), (32, 333, 4), (32, 1025, 0), (32, 97, 2)])
def test_attention_vit_like(dev, rows, N, groups):
    """non-causal, 2 images x 3 heads x 64, N=77 (tails in both q and key tiles), packed qkv rows; 16 and 32 query rows per wave
    (attn_rows), the ViT's N = 1025 (one valid row in the last 32-row block), key groups merged across two row tiles."""
    from vita_amd import _lib, ops
    rng = np.random.default_rng(8)
    B, H, d = 2, 3, 64
    _lib.tune("attn_rows", rows)
    _lib.tune("attn_ksplit", groups)
    try:
        _attention_vit_like(dev, rng, B, H, N, d)
    finally:
        _lib.tune("attn_rows", 0)
        _lib.tune("attn_ksplit", 0)


def _attention_vit_like(dev, rng, B, H, N, d):
    from vita_amd import ops
    qkv = rng.standard_normal((B * N, 3 * H * d), dtype=np.float32)
    t = _dev(qkv, dev)
    out = torch.empty((B * N, H * d), dtype=torch.float32, device=dev)
    ops.attention(t, t[:, H * d:], t[:, 2 * H * d:], out, B=B, Hq=H, Hkv=H, Sq=N, Sk=N, d=d, ldq=3 * H * d, hsq=d,
                  ldk=3 * H * d, hsk=d, ldv=3 * H * d, hsv=d, ldo=H * d, bsq=N * 3 * H * d, bsk=N * 3 * H * d,
                  bso=N * H * d, scale=d ** -0.5)
    for b in range(B):
        r = qkv[b * N:(b + 1) * N].reshape(N, 3, H, d).transpose(1, 2, 0, 3)
        ref = _attn_ref(r[0], r[1], r[2], d ** -0.5)
        assert_close(f"attn vit b{b}", to_np(out[b * N:(b + 1) * N]), ref, atol=ATTN_X3_ATOL)


@pytest.mark.parametrize("impl", [0, 2])
@pytest.mark.parametrize("groups", [1, 2, 4])
def test_attention_key_groups(dev, groups, impl):
    """every key-group instantiation (attn_ksplit: tiles dealt to 1 / 2 / 4 wave groups, merged in group order) gives the
    single-pass result: plain d=64, rel-pos d=64, causal d=128 (4 falls back to 2 there).  impl 0 = the default kernels (plain and
    causal on bf16 x 3 MFMAs: products exact to 2^-17 per term like the GEMMs, tolerance ATTN_X3_ATOL; rel-pos on the fp32 MFMA),
    2 = fp32 MFMA everywhere (fp32 rounding: 2e-5)."""
    from vita_amd import _lib, ops
    rng = np.random.default_rng(80)
    _lib.tune("attn_ksplit", groups)
    _lib.tune("attn_impl", impl)
    tol = ATTN_X3_ATOL if impl == 0 else 2e-5
    try:
        H, N, d = 2, 333, 64
        q, k, v, p = (rng.standard_normal((N, H * d), dtype=np.float32) for _ in range(4))
        bu, bv = rng.standard_normal((H, d), dtype=np.float32), rng.standard_normal((H, d), dtype=np.float32)
        sp = lambda x: x.reshape(N, H, d).transpose(1, 0, 2)
        out = torch.empty((N, H * d), dtype=torch.float32, device=dev)
        kw = dict(B=1, Hq=H, Hkv=H, Sq=N, Sk=N, d=d, ldq=H * d, hsq=d, ldk=H * d, hsk=d, ldv=H * d, hsv=d, ldo=H * d,
                  scale=d ** -0.5)
        ops.attention(_dev(q, dev), _dev(k, dev), _dev(v, dev), out, **kw)
        assert_close(f"plain groups={groups}", to_np(out), _attn_ref(sp(q), sp(k), sp(v), d ** -0.5), atol=tol)
        ops.attention(_dev(q, dev), _dev(k, dev), _dev(v, dev), out, klen=301, p=_dev(p, dev), ldp=H * d, hsp=d,
                      bias_u=_dev(bu, dev), bias_v=_dev(bv, dev), **kw)
        mask = np.broadcast_to(np.arange(N)[None, :] < 301, (N, N))
        ref = _attn_ref(sp(q), sp(k), sp(v), d ** -0.5, mask, sp(p), bu[:, None, :], bv[:, None, :])
        assert_close(f"relpos groups={groups}", to_np(out), ref, atol=5e-5)
        nq, nkv, d2, max_ctx, Sq, pos0 = 4, 2, 128, 400, 150, 170
        Sk = pos0 + Sq
        q2 = rng.standard_normal((Sq, nq * d2), dtype=np.float32)
        kc = rng.standard_normal((nkv, max_ctx, d2), dtype=np.float32)
        vc = rng.standard_normal((nkv, max_ctx, d2), dtype=np.float32)
        out2 = torch.empty((Sq, nq * d2), dtype=torch.float32, device=dev)
        ops.attention(_dev(q2, dev), _dev(kc, dev), _dev(vc, dev), out2, B=1, Hq=nq, Hkv=nkv, Sq=Sq, Sk=Sk, d=d2,
                      ldq=nq * d2, hsq=d2, ldk=d2, hsk=max_ctx * d2, ldv=d2, hsv=max_ctx * d2, ldo=nq * d2,
                      scale=d2 ** -0.5, causal=True, q_off=pos0)
        cm = np.arange(Sk)[None, :] <= (pos0 + np.arange(Sq))[:, None]
        ref2 = _attn_ref(q2.reshape(Sq, nq, d2).transpose(1, 0, 2), kc[:, :Sk], vc[:, :Sk], d2 ** -0.5, cm)
        assert_close(f"causal gqa groups={groups}", to_np(out2), ref2, atol=tol)
    finally:
        _lib.tune("attn_ksplit", 0)
        _lib.tune("attn_impl", 0)


@pytest.mark.parametrize("nq,nkv,causal", [(8, 2, True), (4, 1, True), (8, 2, False)])
@pytest.mark.parametrize("Sq,pos0", [(70, 0), (33, 45), (1, 99), (150, 170), (64, 64), (129, 0)])
@pytest.mark.parametrize("rows,xcd", [(0, 1), (32, 1), (32, 0)], ids=["rows16", "rows32", "rows32-plain-grid"])
def test_attention_flash_form(dev, nq, nkv, causal, Sq, pos0, rows, xcd):
    """k_attn_fa forced (attn_fa = 2; by default it runs when its blocks fill half the chip): d = 128, 4 : 1 head grouping (one block
    = the four query heads of a KV head on the same 16 rows, eight waves = heads x two 32-key halves merged at the end), causal with
    a query offset (chunked prefill) or a key pad mask, K / V in cache layout [nkv][max_ctx][d]; tails in the 16-row blocks, the
    64-key tiles and their halves; rows past the context hold NaNs and must never reach a product.  r06: 32 query rows per wave
    (attn_rows = 32, causal only: what long prompts take by themselves) and the XCD-aware block -> (q tile, KV head) mapping on / off."""
    from vita_amd import _lib, ops
    rng = np.random.default_rng(10 + Sq + nq)
    d, max_ctx = 128, 400
    Sk = pos0 + Sq
    klen = Sk if causal else max(1, Sk - 37)
    q = rng.standard_normal((Sq, nq * d), dtype=np.float32)
    kc = rng.standard_normal((nkv, max_ctx, d), dtype=np.float32)
    vc = rng.standard_normal((nkv, max_ctx, d), dtype=np.float32)
    kc[:, Sk:] = np.nan
    vc[:, Sk:] = np.nan
    if not causal:          # pad mask: rows in [klen, Sk) are caller memory too — masked keys must not be loaded from them
        kc[:, klen:] = np.nan
        vc[:, klen:] = np.nan
    out = torch.full((Sq, nq * d), float("nan"), dtype=torch.float32, device=dev)
    _lib.tune("attn_fa", 2)
    _lib.tune("attn_rows", rows)
    _lib.tune("attn_xcd", xcd)
    try:
        ops.attention(_dev(q, dev), _dev(kc, dev), _dev(vc, dev), out, B=1, Hq=nq, Hkv=nkv, Sq=Sq, Sk=Sk, d=d, ldq=nq * d,
                      hsq=d, ldk=d, hsk=max_ctx * d, ldv=d, hsv=max_ctx * d, ldo=nq * d, scale=d ** -0.5, causal=causal, q_off=pos0,
                      klen=klen)
    finally:
        _lib.tune("attn_fa", 1)
        _lib.tune("attn_rows", 0)
        _lib.tune("attn_xcd", 1)
    mask = (np.arange(Sk)[None, :] <= (pos0 + np.arange(Sq))[:, None]) if causal else np.broadcast_to(np.arange(Sk)[None, :] < klen, (Sq, Sk))
    ref = _attn_ref(q.reshape(Sq, nq, d).transpose(1, 0, 2), np.nan_to_num(kc[:, :Sk]), np.nan_to_num(vc[:, :Sk]), d ** -0.5, mask)
    assert_close(f"flash form nq={nq} causal={causal} Sq={Sq} pos0={pos0}", to_np(out), ref, atol=ATTN_X3_ATOL)


def test_attention_big_scores(dev):
    """large score range exercises the online-softmax rescale branch (running max jumps)."""
    from vita_amd import ops
    rng = np.random.default_rng(9)
    H, N, d = 2, 130, 64
    q = rng.standard_normal((N, H * d), dtype=np.float32) * 3
    k = rng.standard_normal((N, H * d), dtype=np.float32) * 3
    k[97] *= 4.0  # spike late in the key order
    v = rng.standard_normal((N, H * d), dtype=np.float32)
    out = torch.empty((N, H * d), dtype=torch.float32, device=dev)
    ops.attention(_dev(q, dev), _dev(k, dev), _dev(v, dev), out, B=1, Hq=H, Hkv=H, Sq=N, Sk=N, d=d, ldq=H * d, hsq=d,
                  ldk=H * d, hsk=d, ldv=H * d, hsv=d, ldo=H * d, scale=d ** -0.5)
    sp = lambda x: x.reshape(N, H, d).transpose(1, 0, 2)
    assert_close("attn big scores", to_np(out), _attn_ref(sp(q), sp(k), sp(v), d ** -0.5), atol=4 * ATTN_X3_ATOL)   # scores x 9


@pytest.mark.parametrize("Sq,pos0", [(70, 0), (33, 45), (1, 99)])
def test_attention_causal_gqa(dev, Sq, pos0):
    """Mixtral prefill shape on the direct kernel: 4 q-heads / 2 kv-heads x 128 (a 2 : 1 grouping the flash form does not take),
    K/V in cache layout [nkv][max_ctx][128]."""
    from vita_amd import _lib, ops
    rng = np.random.default_rng(10 + Sq)
    nq, nkv, d, max_ctx = 4, 2, 128, 160
    Sk = pos0 + Sq
    q = rng.standard_normal((Sq, nq * d), dtype=np.float32)
    kc = rng.standard_normal((nkv, max_ctx, d), dtype=np.float32)
    vc = rng.standard_normal((nkv, max_ctx, d), dtype=np.float32)
    out = torch.empty((Sq, nq * d), dtype=torch.float32, device=dev)
    ops.attention(_dev(q, dev), _dev(kc, dev), _dev(vc, dev), out, B=1, Hq=nq, Hkv=nkv, Sq=Sq, Sk=Sk, d=d, ldq=nq * d,
                  hsq=d, ldk=d, hsk=max_ctx * d, ldv=d, hsv=max_ctx * d, ldo=nq * d, scale=d ** -0.5, causal=True,
                  q_off=pos0)
    mask = np.arange(Sk)[None, :] <= (pos0 + np.arange(Sq))[:, None]
    ref = _attn_ref(q.reshape(Sq, nq, d).transpose(1, 0, 2), kc[:, :Sk], vc[:, :Sk], d ** -0.5, mask)
    assert_close(f"attn causal gqa Sq={Sq} pos0={pos0}", to_np(out), ref, atol=ATTN_X3_ATOL)


@pytest.mark.parametrize("klen,chunk,left", [(87, 0, -1), (60, 0, -1), (87, 16, 2), (87, 7, -1)])
def test_attention_relpos_masks(dev, klen, chunk, left):
    """Whale rel-pos scores ((q+u)k^T + (q+v)p^T)/sqrt(d), no rel-shift, pad + chunk masks
    (attention.py:380-409, utils.py:88-103)."""
    from vita_amd import ops
    rng = np.random.default_rng(11)
    H, T, d = 2, 87, 64
    q, k, v, p = (rng.standard_normal((T, H * d), dtype=np.float32) for _ in range(4))
    bu, bv = rng.standard_normal((H, d), dtype=np.float32), rng.standard_normal((H, d), dtype=np.float32)
    out = torch.empty((T, H * d), dtype=torch.float32, device=dev)
    k_dev, v_dev = k.copy(), v.copy()
    k_dev[klen:] = np.nan            # padded key rows are caller memory: masked keys must not be loaded from them
    v_dev[klen:] = np.nan
    ops.attention(_dev(q, dev), _dev(k_dev, dev), _dev(v_dev, dev), out, B=1, Hq=H, Hkv=H, Sq=T, Sk=T, d=d, ldq=H * d, hsq=d,
                  ldk=H * d, hsk=d, ldv=H * d, hsv=d, ldo=H * d, scale=d ** -0.5, klen=klen, chunk=chunk, left=left,
                  p=_dev(p, dev), ldp=H * d, hsp=d, bias_u=_dev(bu, dev), bias_v=_dev(bv, dev))
    mask = np.broadcast_to(np.arange(T)[None, :] < klen, (T, T)).copy()
    if chunk > 0:
        for i in range(T):
            start = 0 if left < 0 else max((i // chunk - left) * chunk, 0)
            end = min((i // chunk + 1) * chunk, T)
            mask[i, :start] = False
            mask[i, end:] = False
    sp = lambda x: x.reshape(T, H, d).transpose(1, 0, 2)
    ref = _attn_ref(sp(q), sp(k), sp(v), d ** -0.5, mask, sp(p), bu[:, None, :], bv[:, None, :])
    assert_close(f"attn relpos klen={klen} chunk={chunk}", to_np(out), ref, atol=5e-5)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [128, 1024, 2048, 4096])
def test_layernorm_rmsnorm(dev, cols):
    from vita_amd import ops
    rng = np.random.default_rng(12)
    rows = 37
    x = rng.standard_normal((rows, cols), dtype=np.float32) * 2 + 0.5
    w, b = _w(rng, cols, std=1.0), _w(rng, cols, std=0.5)
    x64 = x.astype(np.float64)
    mu, var = x64.mean(-1, keepdims=True), x64.var(-1, keepdims=True)
    ref = (x64 - mu) / np.sqrt(var + 1e-5) * w + b
    assert_close("layernorm", to_np(ops.layernorm(_dev(x, dev), _dev(w, dev), _dev(b, dev), 1e-5)), ref, atol=2e-5)
    assert_close("layernorm relu*32", to_np(ops.layernorm(_dev(x, dev), _dev(w, dev), _dev(b, dev), 1e-5, act="relu",
                                                          post_scale=32.0)), np.maximum(ref, 0) * 32.0, atol=5e-4)
    rref = x64 / np.sqrt((x64 ** 2).mean(-1, keepdims=True) + 1e-5) * w
    assert_close("rmsnorm", to_np(ops.rmsnorm(_dev(x, dev), _dev(w, dev), 1e-5)), rref, atol=2e-5)


def test_vit_front_back(dev):
    """patchify (conv 14x14/14 as GEMM rows), CLS/pos assemble, pixel shuffle vs torch-free numpy
    restatements of modeling_intern_vit.py:109-121 and internvit_encoder.py:42-53."""
    from vita_amd import ops
    rng = np.random.default_rng(13)
    n, img, P, C = 2, 56, 14, 32
    g = img // P
    pix = rng.standard_normal((n, 3, img, img), dtype=np.float32)
    kpad = 640
    got = to_np(ops.vit_patchify(_dev(pix, dev), P, kpad))
    ref = pix.reshape(n, 3, g, P, g, P).transpose(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * P * P)
    assert_close("patchify", got[:, :3 * P * P], ref, atol=0)
    assert np.all(got[:, 3 * P * P:] == 0)
    patches = rng.standard_normal((n * g * g, C), dtype=np.float32)
    cls, pos = _w(rng, C, std=1.0), _w(rng, g * g + 1, C, std=1.0)
    x = to_np(ops.vit_assemble(_dev(patches, dev), _dev(cls, dev, torch.bfloat16), _dev(pos, dev, torch.bfloat16), n,
                               g * g + 1, C)).reshape(n, g * g + 1, C)
    xref = np.concatenate([np.broadcast_to(cls, (n, 1, C)), patches.reshape(n, g * g, C)], 1) + pos[None]
    assert_close("assemble", x, xref, atol=1e-6)
    # pixel shuffle reference = the reference's view/permute chain
    f = (xref[:, 1:] * 0.5).reshape(n, g, g, C).astype(np.float32)
    t = f.reshape(n, g, g // 2, 2 * C).transpose(0, 2, 1, 3).reshape(n, g // 2, g // 2, 4 * C).transpose(0, 2, 1, 3)
    got = to_np(ops.vit_pixel_shuffle(_dev(xref.reshape(-1, C).astype(np.float32), dev), n, g, C, 0.5))
    assert_close("pixel_shuffle", got, t.reshape(n, (g // 2) ** 2, 4 * C), atol=1e-6)


def test_audio_conv1(dev):
    from vita_amd import ops
    rng = np.random.default_rng(14)
    T, F, C = 41, 80, 48
    feats = rng.standard_normal((T, F), dtype=np.float32) * 3 + 10
    mean, istd = rng.standard_normal(F).astype(np.float32) + 10, (rng.random(F).astype(np.float32) + 0.5)
    w, b = _w(rng, C, 1, 3, 3, std=0.3), _w(rng, C, std=0.3)
    out, T1, F1 = ops.audio_conv1(_dev(feats, dev), _dev(mean, dev), _dev(istd, dev),
                                  _dev(w.reshape(C, 9), dev, torch.bfloat16), _dev(b, dev))
    xn = ((feats - mean) * istd).astype(np.float64)
    ref = np.zeros((T1, F1, C))
    for t in range(T1):
        for f in range(F1):
            ref[t, f] = np.einsum("hw,chw->c", xn[2 * t:2 * t + 3, 2 * f:2 * f + 3], w[:, 0].astype(np.float64)) + b
    assert_close("audio conv1", to_np(out).reshape(T1, F1, C), np.maximum(ref, 0), atol=1e-4)


def test_embed_splice(dev):
    from vita_amd import ops
    rng = np.random.default_rng(15)
    H, V = 256, 50
    emb = _w(rng, V, H, std=1.0)
    img = rng.standard_normal((8, H), dtype=np.float32)
    aud = rng.standard_normal((5, H), dtype=np.float32)
    kind = np.array([0, 0, 1, 1, 1, 0, 2, 2, 0], np.int32)
    idx = np.array([3, 49, 0, 1, 7, 10, 4, 0, 0], np.int32)
    got = to_np(ops.embed_splice(_dev(kind, dev, torch.int32), _dev(idx, dev, torch.int32),
                                 _dev(emb, dev, torch.bfloat16), _dev(img, dev), _dev(aud, dev), H))
    ref = np.stack([(emb, img, aud)[k][i] for k, i in zip(kind, idx)])
    assert_close("embed_splice", got, ref, atol=0)


# ---- batch-1 decode operators, one C entry each against oracle/mixtral.py ------------------
def _moe_weights(rng, E, I, H):
    return dict(gate=_w(rng, E, H, std=0.2), w1=_w(rng, E, I, H), w3=_w(rng, E, I, H), w2=_w(rng, E, H, I))


@pytest.mark.parametrize("E,H,rows", [(8, 4096, 5), (4, 256, 37), (2, 128, 1)])
def test_router_top2_vs_oracle(dev, E, H, rows):
    from oracle import mixtral as om
    from vita_amd import ops
    rng = np.random.default_rng(E * 100 + rows)
    x = rng.standard_normal((rows, H), dtype=np.float32)
    g = _w(rng, E, H, std=0.1)
    ids, wts, probs = ops.router_top2(_dev(x, dev), _dev(g, dev, torch.bfloat16), want_probs=True)
    ridx, rval = om.router(x, g)
    assert to_np(ids).astype(np.int64).tolist() == ridx.tolist()
    assert_close("router weights", to_np(wts), rval, atol=2e-6)
    assert_close("router softmax", to_np(probs), om.softmax((x @ g.T).astype(np.float32)), atol=2e-6)


@pytest.mark.parametrize("E,I,H", [(8, 14336, 4096), (4, 512, 256)])
def test_moe_decode_vs_oracle(dev, E, I, H):
    """post_attention_layernorm + block_sparse_moe of one token (vh_moe_decode) vs the oracle's rmsnorm + moe, with and
    without the deferred residual (delta)."""
    from oracle import mixtral as om
    from vita_amd import ops
    rng = np.random.default_rng(I)
    lw = _moe_weights(rng, E, I, H)
    x = rng.standard_normal(H, dtype=np.float32)
    d = rng.standard_normal(H, dtype=np.float32) * 0.1
    nw = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    dw = {k: _dev(v, dev, torch.bfloat16) for k, v in lw.items()}
    for delta in (None, d):
        xin = x if delta is None else x + delta
        ref, ridx, rval = om.moe(om.rmsnorm(xin[None], nw, 1e-5), lw)
        y, route = ops.moe_decode(_dev(x, dev), _dev(nw, dev), 1e-5, dw["gate"], dw["w1"], dw["w3"], dw["w2"],
                                  delta=None if delta is None else _dev(delta, dev))
        r = to_np(route.view(torch.int32)).tolist()
        assert r[:2] == ridx[0].tolist()
        w = np.array(r[2:], np.int32).view(np.float32)
        assert_close("routing weights", w, rval[0], atol=2e-6)
        assert_close(f"moe_decode E={E} I={I}", to_np(y), ref[0], atol=1e-3 * max(1.0, float(np.abs(ref).max())), rtol=1e-4)


def test_rope_kv_append_and_attn_decode_vs_oracle(dev):
    """vh_rope_kv_append fills the cache for a 70-token prefix (two 64-key tiles), vh_attn_decode appends token 70 and attends
    over [0, 70]: RoPE'd q / k, the cache rows and the attention output vs oracle apply_rope / attention."""
    from oracle import mixtral as om
    from vita_amd import ops
    from vita_amd.engine import rope_tables
    rng = np.random.default_rng(77)
    nq, nkv, d, S, max_ctx = 8, 2, 128, 70, 192
    nqkv = (nq + 2 * nkv) * d
    qkv = rng.standard_normal((S + 1, nqkv), dtype=np.float32)
    cos, sin = rope_tables(max_ctx, d, 1e6)
    kc = torch.zeros((nkv, max_ctx, d), dtype=torch.float32, device=dev)
    vc = torch.zeros_like(kc)
    dcos, dsin = _dev(cos, dev), _dev(sin, dev)
    q = ops.rope_kv_append(_dev(qkv[:S], dev), kc, vc, dcos, dsin, 0, nq, nkv)
    c2, s2 = om.rope_cos_sin(np.arange(S + 1), d, 1e6)
    qh = qkv[:, :nq * d].reshape(S + 1, nq, d).transpose(1, 0, 2)
    kh = qkv[:, nq * d:(nq + nkv) * d].reshape(S + 1, nkv, d).transpose(1, 0, 2)
    vh = qkv[:, (nq + nkv) * d:].reshape(S + 1, nkv, d).transpose(1, 0, 2)
    qr, kr = om.apply_rope(qh, c2, s2), om.apply_rope(kh, c2, s2)
    # (the engine's tables are built in fp32 from float32(theta) ** ..., the oracle's inv_freq in fp64 then rounded: HF's order;
    # the angle differs by ~1e-6 relative at position 69: a few 1e-5 on values up to 4)
    assert_close("roped q", to_np(q), qr[:, :S].transpose(1, 0, 2).reshape(S, nq * d), atol=5e-5)
    assert_close("k cache", to_np(kc)[:, :S], kr[:, :S], atol=5e-5)
    assert_close("v cache", to_np(vc)[:, :S], vh[:, :S], atol=0)
    out = ops.attn_decode(_dev(qkv[S], dev), kc, vc, S, dcos, dsin, nq, nkv, d ** -0.5)
    ref = om.attention(qr[:, S:S + 1], kr, vh, S)
    assert_close("k appended", to_np(kc)[:, S], kr[:, S], atol=5e-5)
    assert_close("attn_decode", to_np(out), ref[0], atol=5e-5)


@pytest.mark.parametrize("V,H", [(51760, 4096), (1000, 256)])
def test_lmhead_argmax_vs_oracle(dev, V, H):
    from oracle import mixtral as om
    from vita_amd import ops
    rng = np.random.default_rng(V)
    x = rng.standard_normal(H, dtype=np.float32)
    d = rng.standard_normal(H, dtype=np.float32) * 0.1
    nw = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    w = _w(rng, V, H)
    ref = (om.rmsnorm((x + d)[None], nw, 1e-5) @ w.T).astype(np.float32)[0]
    logits, tok = ops.lmhead_argmax(_dev(x, dev), _dev(nw, dev), 1e-5, _dev(w, dev, torch.bfloat16), delta=_dev(d, dev))
    assert_close("lm_head logits", to_np(logits), ref, atol=1e-3)
    assert int(tok.item()) == int(np.argmax(ref))
    # ties: the lowest index wins (torch.argmax / HF greedy)
    w2 = w.copy(); w2[7] = w2[3]
    _, tok2 = ops.lmhead_argmax(_dev(w2[3].astype(np.float32) * 50, dev), _dev(np.ones(H, np.float32), dev), 1e-5, _dev(w2, dev, torch.bfloat16))
    lg2 = (om.rmsnorm((w2[3].astype(np.float32) * 50)[None], np.ones(H, np.float32), 1e-5) @ w2.T)[0]
    assert int(tok2.item()) == int(np.argmax(lg2)) and int(tok2.item()) in (3, int(np.argmax(lg2)))


# ---- past 4096 tokens: the range a 16-frame video prompt reaches (tokenizer_model_max_length = 4600) ----------------------
# vh_attn_decode merges its 64-key splits in rounds of 64 lanes (a second round from pos 4096 on), and a paged sequence past 4096
# tokens has more than 64 pages.  The references take the ENGINE's RoPE rows (vita_amd/engine.py rope_tables): the oracle's table
# computes inv_freq in another order and differs from it by one fp32 ulp of the angle (up to 4.9e-4 on cos / sin past 4096), so a
# bit-exact target does not exist and the kernels, not the table definitions, are what these tests are about.
LONG_CTX = 73 * 64          # 4672 rows: 73 splits / pages, room for the model's 4600-token limit plus decode steps


def _rope64(x, c, s):
    """rotate-half RoPE of x [..., 128] in fp64 with one position's engine row c, s [64] (modeling_mixtral.py:203-241)."""
    x = np.asarray(x, np.float64)
    a, b = x[..., :64], x[..., 64:]
    c, s = np.asarray(c, np.float64), np.asarray(s, np.float64)
    return np.concatenate([a * c - b * s, b * c + a * s], -1)


def _unrope64(y, c, s):
    """inverse of _rope64: the pre-RoPE row whose rotation is y."""
    y = np.asarray(y, np.float64)
    a, b = y[..., :64], y[..., 64:]
    return np.concatenate([a * c + b * s, b * c - a * s], -1)


def _to_pages(logical, perm):
    """[nkv, n_pages * 64, d] in sequence order -> the physical pool with logical page p stored in page perm[p] (perm None: as is)."""
    if perm is None:
        return logical.copy()
    phys = np.empty_like(logical)
    for p, q in enumerate(perm):
        phys[:, q * 64:(q + 1) * 64] = logical[:, p * 64:(p + 1) * 64]
    return phys


def _from_pages(phys, perm):
    if perm is None:
        return phys
    return np.concatenate([phys[:, q * 64:(q + 1) * 64] for q in perm], 1)


def _steer(q_roped, target):
    """key row k [128] with q_g . k == target exactly (fp64) for every query head g of a KV group (least-norm solution)."""
    Q = np.asarray(q_roped, np.float64)
    return Q.T @ np.linalg.solve(Q @ Q.T, np.full(Q.shape[0], float(target)))


_ATTN_PATTERNS = {"late-max-20": (70 * 64 + 9, 25.0, None), "late-max-100": (70 * 64 + 9, 100.0, None),
                  "late-splits-underflow": (5, 60.0, -60.0)}


def _steer_pattern(rng, pattern, qkv, kl, pos, c, s, nq, nkv, scale):
    """the score patterns of test_attn_decode_long_context, written into the logical K rows kl [nkv, rows, 128] and (underflow) the
    appended key of qkv, both in place."""
    if pattern == "random":
        return
    d, G = 128, nq // nkv
    qr = _rope64(qkv[:nq * d].reshape(nq, d), c, s)
    hi_key, hi, lo = _ATTN_PATTERNS[pattern]
    for h in range(nkv):
        Qg = qr[h * G:(h + 1) * G]
        kl[h, hi_key] = _steer(Qg, hi / scale).astype(np.float32)
        if lo is not None:
            kl[h, 65 * 64:pos] = (_steer(Qg, lo / scale)[None, :] + 0.1 * rng.standard_normal((pos - 65 * 64, d))).astype(np.float32)
            kn = _unrope64(_steer(Qg, lo / scale), c, s)          # the appended key lies in split 71 as well
            qkv[(nq + h) * d:(nq + h + 1) * d] = kn.astype(np.float32)


def _attn_decode_ref(qkv, kl, vl, pos, c, s, nq, nkv, scale, pattern="random"):
    """fp64 attention of one token at `pos` over the logical rows kl / vl [nkv, >= pos, 128] and its own appended row -> (output
    [nq * 128], RoPE'd appended K rows [nkv, 128], appended V rows); asserts that a steered pattern is what it claims to be."""
    d, G = 128, nq // nkv
    qr = _rope64(qkv[:nq * d].reshape(nq, d), c, s)
    k_new = _rope64(qkv[nq * d:(nq + nkv) * d].reshape(nkv, d), c, s)
    v_new = qkv[(nq + nkv) * d:].reshape(nkv, d)
    K = kl[:, :pos + 1].astype(np.float64)
    V = vl[:, :pos + 1].astype(np.float64)
    K[:, pos], V[:, pos] = k_new, v_new
    ref = np.empty(nq * d)
    for hq in range(nq):
        sc = K[hq // G] @ qr[hq] * scale
        if pattern == "late-splits-underflow":
            assert sc.max() - sc[65 * 64:].max() > 110          # the late splits' weights are exactly 0 in fp32
        elif pattern != "random":
            hi_key = _ATTN_PATTERNS[pattern][0]
            assert np.argmax(sc) == hi_key and sc[hi_key] - np.delete(sc, hi_key).max() > 19
        p = np.exp(sc - sc.max())
        ref[hq * d:(hq + 1) * d] = (p / p.sum()) @ V[hq // G]
    return ref, k_new, v_new


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("nq,nkv", [(32, 8), (8, 2)])
@pytest.mark.parametrize("pos,pattern", [(63, "random"), (64, "random"), (127, "random"), (4095, "random"), (4096, "random"),
                                         (4097, "random"), (4600, "random"), (4671, "random"), (4600, "late-max-20"),
                                         (4600, "late-max-100"), (4600, "late-splits-underflow")])
def test_attn_decode_long_context(dev, nq, nkv, pos, pattern, paged):
    """vh_attn_decode (the k_dec_attn launches; the one-launch block and the batched kernel share dec_attn_finish) across the
    64-split boundary of its merge — nsplit = ceil((pos + 1) / 64) > 64 from pos 4096 on takes a second round of 64 lanes for the
    split statistics and partials — and across 73 pages, contiguous or through a fixed random permutation of the pages (`table`).
    Cache rows are random (no prefill needed); checked against fp64: the output, the appended RoPE'd K row and the appended V row.
    Score patterns that pin the merge (pos 4600: 72 splits, 8 in the second lane round):
      late-max-20   one key of split 70 scores 25 against |s| < ~4 elsewhere: the global max lives only in the second round;
      late-max-100  the same key 100 above the rest: a merge whose running max M skipped the second round would weight that split
                    by exp(> 88) = inf (at a gap of 20 such a merge is still exact up to rounding: only overflow shows it);
      late-splits-underflow  the max sits in split 0 (+60), every key of splits >= 65 (the appended one included) scores -60:
                    their merge weights exp(-120) are exactly 0 and must drop out without a NaN."""
    from vita_amd import ops
    from vita_amd.engine import rope_tables
    rng = np.random.default_rng(pos * 7 + nq + (1 if paged else 0) + 1000 * len(pattern))
    d, G = 128, nq // nkv
    cos, sin = rope_tables(LONG_CTX, d, 1e6)
    c, s = cos[pos].astype(np.float64), sin[pos].astype(np.float64)
    scale = d ** -0.5
    qkv = rng.standard_normal((nq + 2 * nkv) * d, dtype=np.float32)
    std = 1.0 if pattern == "random" else 0.1
    kl = (rng.standard_normal((nkv, LONG_CTX, d), dtype=np.float32) * std).astype(np.float32)
    vl = rng.standard_normal((nkv, LONG_CTX, d), dtype=np.float32)
    _steer_pattern(rng, pattern, qkv, kl, pos, c, s, nq, nkv, scale)
    perm = rng.permutation(LONG_CTX // 64) if paged else None
    table = _dev(perm, dev, torch.int32) if paged else None
    kc, vc = _dev(_to_pages(kl, perm), dev), _dev(_to_pages(vl, perm), dev)
    out = ops.attn_decode(_dev(qkv, dev), kc, vc, pos, _dev(cos, dev), _dev(sin, dev), nq, nkv, scale, table=table)
    ref, k_new, v_new = _attn_decode_ref(qkv, kl, vl, pos, c, s, nq, nkv, scale, pattern)
    kb, vb = _from_pages(to_np(kc), perm), _from_pages(to_np(vc), perm)
    assert_close(f"appended K row at {pos}", kb[:, pos], k_new, atol=5e-5)
    assert_close(f"appended V row at {pos}", vb[:, pos], v_new, atol=0)
    assert_close(f"attn_decode pos={pos} {pattern}", to_np(out), ref, atol=5e-5)


# ---- the batched decode attention (vh_attn_decode_batch: k_decb_attn, the attention launch of a batched decode iteration) ---------
_ATTN_BATCHES = [
    ((8, 2), [63], None), ((32, 8), [63], None),
    ((8, 2), [64, 63], None),
    ((8, 2), [0, 127, 4095], None),
    ((8, 2), [4600, 37, 4096, 4097], None),
    ((8, 2), [37, 4097, 4096, 4600], None),                                                   # the longest last
    ((8, 2), [4600] * 4, ["random", "random", "late-max-100", "late-splits-underflow"]),
    ((32, 8), [4600] * 4, ["random", "random", "late-max-100", "late-splits-underflow"]),
]


def _attn_batch_setup(dev, nq, nkv, positions, patterns, seed):
    """n sequences over ONE pool: every sequence owns ceil((pos + 1) / 64) pages dealt from one random permutation of the pool's
    pages (so the sequences' pages interleave; 3 pages belong to nobody), random rows everywhere — stale rows past a sequence's
    position in its last page included.  -> inputs on the device and the fp64 references per member."""
    from vita_amd.engine import rope_tables
    rng = np.random.default_rng(seed)
    d, n = 128, len(positions)
    scale = d ** -0.5
    cos, sin = rope_tables(LONG_CTX, d, 1e6)
    need = [p // 64 + 1 for p in positions]
    n_pages = sum(need) + 3
    perm = rng.permutation(n_pages)
    pages = [perm[sum(need[:b]):sum(need[:b + 1])] for b in range(n)]
    kp = rng.standard_normal((nkv, n_pages * 64, d), dtype=np.float32)
    vp = rng.standard_normal((nkv, n_pages * 64, d), dtype=np.float32)
    members = []
    for b, pos in enumerate(positions):
        pattern = patterns[b] if patterns else "random"
        c, s = cos[pos].astype(np.float64), sin[pos].astype(np.float64)
        qkv = rng.standard_normal((nq + 2 * nkv) * d, dtype=np.float32)
        std = 1.0 if pattern == "random" else 0.1
        kl = (rng.standard_normal((nkv, need[b] * 64, d), dtype=np.float32) * std).astype(np.float32)
        vl = rng.standard_normal((nkv, need[b] * 64, d), dtype=np.float32)
        _steer_pattern(rng, pattern, qkv, kl, pos, c, s, nq, nkv, scale)
        for p, q in enumerate(pages[b]):
            kp[:, q * 64:(q + 1) * 64] = kl[:, p * 64:(p + 1) * 64]
            vp[:, q * 64:(q + 1) * 64] = vl[:, p * 64:(p + 1) * 64]
        ref, k_new, v_new = _attn_decode_ref(qkv, kl, vl, pos, c, s, nq, nkv, scale, pattern)
        members.append(dict(pos=pos, qkv=_dev(qkv, dev), table=_dev(pages[b], dev, torch.int32), ref=ref, k_new=k_new, v_new=v_new,
                            row=int(pages[b][pos // 64]) * 64 + pos % 64))
    # the pages interleave: no sequence of several pages holds a contiguous ascending run
    assert all(len(pg) < 2 or not np.array_equal(pg, np.arange(pg[0], pg[0] + len(pg))) for pg in pages)
    return dict(kc=_dev(kp, dev), vc=_dev(vp, dev), cos=_dev(cos, dev), sin=_dev(sin, dev), scale=scale, members=members)


@pytest.mark.parametrize("heads,positions,patterns", _ATTN_BATCHES,
                         ids=[f"{h[0]}-{h[1]}-" + "-".join(map(str, p)) + ("-patterns" if pt else "") for h, p, pt in _ATTN_BATCHES])
def test_attn_decode_batch(dev, heads, positions, patterns):
    """vh_attn_decode_batch = one k_decb_attn launch, grid (nkv, max splits of the batch, n): sequences of very different lengths
    (73 splits next to 1: most blocks of the short ones leave at once), the longest in the first and in the last lane, a lone
    sequence, positions on both sides of a page boundary and of the 64-split boundary of the merge, and the merge patterns of
    test_attn_decode_long_context in lanes 2 and 3 next to random neighbours.  Per member against fp64: the output and the appended
    K row within the batch-1 operator's 5e-5, the appended V row exactly.  Every other row of the pool stays bit-unchanged.  The
    kernel promises the batch-1 arithmetic per sequence: every output, and the pool, are BIT-equal to vh_attn_decode run on the
    members one after the other (own scratch, a copy of the pool).  A second call on the same scratch gives the same bits (the
    tickets were left reset)."""
    from vita_amd import ops
    nq, nkv = heads
    t = _attn_batch_setup(dev, nq, nkv, positions, patterns, seed=sum(positions) * 3 + nq + len(positions))
    ms, kc, vc = t["members"], t["kc"], t["vc"]
    k0, v0 = kc.clone(), vc.clone()
    scratch = ops.attn_decode_scratch(len(ms), nq, nkv, kc.shape[1], dev)
    for sc in scratch:
        sc[3].fill_(float("nan"))
    args = ([m["qkv"] for m in ms], kc, vc, [m["pos"] for m in ms], t["cos"], t["sin"], nq, nkv, t["scale"], [m["table"] for m in ms])
    outs = [o.clone() for o in ops.attn_decode_batch(*args, scratch=scratch)]
    torch.cuda.synchronize()
    assert all(int(sc[2].abs().sum().item()) == 0 for sc in scratch), "tickets were not left at zero"
    kg, vg = to_np(kc), to_np(vc)
    for b, m in enumerate(ms):
        what = f"member {b} of {positions} at pos {m['pos']}"
        assert_close(f"attn_decode_batch {what}", to_np(outs[b]), m["ref"], atol=5e-5)
        assert_close(f"appended K row, {what}", kg[:, m["row"]], m["k_new"], atol=5e-5)
        assert_close(f"appended V row, {what}", vg[:, m["row"]], m["v_new"], atol=0)
    rows = torch.tensor([m["row"] for m in ms], device=dev)
    k0[:, rows], v0[:, rows] = kc[:, rows], vc[:, rows]
    assert torch.equal(k0, kc) and torch.equal(v0, vc), "a pool row other than the appended ones changed"
    # the members alone, one after the other, on a copy of the pool as it was before the call
    k1, v1 = k0.clone(), v0.clone()
    k1[:, rows], v1[:, rows] = float("nan"), float("nan")               # (the appended rows are written, never read)
    for b, m in enumerate(ms):
        solo = ops.attn_decode(m["qkv"], k1, v1, m["pos"], t["cos"], t["sin"], nq, nkv, t["scale"], table=m["table"])
        assert torch.equal(solo, outs[b]), f"member {b} of {positions}: the batched output is not the batch-1 operator's, bit for bit"
    assert torch.equal(k1, kc) and torch.equal(v1, vc), "the pool after the batched call is not the pool after the batch-1 calls"
    again = ops.attn_decode_batch(*args, scratch=scratch)
    for b in range(len(ms)):
        assert torch.equal(again[b], outs[b]), f"member {b} of {positions}: a second call on the same scratch differs"
    assert torch.equal(k1, kc) and torch.equal(v1, vc)


def test_attn_decode_batch_refuses_bad_arguments(dev):
    """n outside [1, VH_BMAX = 4], a position outside the pool, null pointers and scratch shared between two members are refused
    before anything is launched: outputs, tickets and pool stay as they were."""
    import ctypes as C
    from vita_amd import _lib, ops
    nq, nkv = 8, 2
    t = _attn_batch_setup(dev, nq, nkv, [70, 5, 64, 130, 9], None, seed=3)
    ms, kc, vc = t["members"], t["kc"], t["vc"]
    max_ctx = kc.shape[1]
    k0, v0 = kc.clone(), vc.clone()
    scratch = ops.attn_decode_scratch(5, nq, nkv, max_ctx, dev)
    for sc in scratch:
        sc[3].fill_(float("nan"))

    def call(idx, positions=None, scr=None, tables=None):
        positions = [ms[i]["pos"] for i in idx] if positions is None else positions
        return ops.attn_decode_batch([ms[i]["qkv"] for i in idx], kc, vc, positions, t["cos"], t["sin"], nq, nkv, t["scale"],
                                     [ms[i]["table"] for i in idx] if tables is None else tables,
                                     scratch=[scratch[i] for i in idx] if scr is None else scr)

    with pytest.raises(_lib.VitaHipError, match="outside"):
        call([0, 1, 2, 3, 4])                                           # five sequences
    with pytest.raises(_lib.VitaHipError, match="outside"):
        call([])
    for bad in (max_ctx, -1, 1 << 30):
        with pytest.raises(_lib.VitaHipError, match="outside the cache"):
            call([0, 1], positions=[ms[0]["pos"], bad])
    with pytest.raises(_lib.VitaHipError, match="share"):
        call([0, 1], scr=[scratch[0], scratch[0]])
    with pytest.raises(_lib.VitaHipError, match="share"):
        call([0, 1, 2], scr=[scratch[0], scratch[1], scratch[0][:3] + (scratch[2][3],)])
    # null pointers: the arrays themselves, an entry of them (a null page table is the contiguous layout and is accepted)
    lib = _lib.load()
    two = lambda ts: (C.c_void_p * 2)(*[tt.data_ptr() if tt is not None else None for tt in ts])
    arrs = dict(qkv=two([ms[0]["qkv"], ms[1]["qkv"]]), table=two([ms[0]["table"], ms[1]["table"]]), part_o=two([scratch[0][0], scratch[1][0]]),
                part_ml=two([scratch[0][1], scratch[1][1]]), tickets=two([scratch[0][2], scratch[1][2]]),
                attn_out=two([scratch[0][3], scratch[1][3]]))
    pos = (C.c_int * 2)(ms[0]["pos"], ms[1]["pos"])

    def raw(**over):
        a = dict(arrs, pos=pos, kc=kc.data_ptr(), vc=vc.data_ptr(), cos=t["cos"].data_ptr(), sin=t["sin"].data_ptr())
        a.update(over)
        return lib.vh_attn_decode_batch(2, a["qkv"], a["kc"], a["vc"], a["pos"], a["cos"], a["sin"], nq, nkv, max_ctx, t["scale"], a["table"],
                                        a["part_o"], a["part_ml"], a["tickets"], a["attn_out"], None)

    for name in ("qkv", "kc", "vc", "pos", "cos", "sin", "table", "part_o", "part_ml", "tickets", "attn_out"):
        assert raw(**{name: None}) == -2 and b"null pointer" in lib.vh_last_error(), name          # VH_E_ARG
    for name, ts in (("qkv", [ms[0]["qkv"], None]), ("part_o", [scratch[0][0], None]), ("part_ml", [None, scratch[1][1]]),
                     ("tickets", [scratch[0][2], None]), ("attn_out", [None, scratch[1][3]])):
        assert raw(**{name: two(ts)}) == -2 and b"null pointer" in lib.vh_last_error(), name
    torch.cuda.synchronize()
    assert torch.equal(k0, kc) and torch.equal(v0, vc), "a refused call wrote to the pool"
    assert all(bool(torch.isnan(sc[3]).all()) and int(sc[2].abs().sum().item()) == 0 for sc in scratch), "a refused call wrote an output"
    outs = call([0, 1])                                                  # and the same arguments, all valid, are accepted
    torch.cuda.synchronize()
    for b in (0, 1):
        assert_close(f"member {b} after the refusals", to_np(outs[b]), ms[b]["ref"], atol=5e-5)


@pytest.mark.parametrize("nq,nkv", [(32, 8), (8, 2)])
def test_rope_kv_append_paged_across_page_64(dev, nq, nkv):
    """vh_rope_kv_append through a page table: 12 rows at positions 4090 ... 4101 cross the page boundary at 4096 (logical page 64,
    the 65th) and land in two physical pages of a fixed random permutation of 73; q, and the K / V rows read back through the table,
    against fp64 RoPE with the engine's rows.  Every other row of the pool must be left as it was."""
    from vita_amd import ops
    from vita_amd.engine import rope_tables
    rng = np.random.default_rng(4090 + nq)
    d, pos0, n = 128, 4090, 12
    cos, sin = rope_tables(LONG_CTX, d, 1e6)
    qkv = rng.standard_normal((n, (nq + 2 * nkv) * d), dtype=np.float32)
    perm = rng.permutation(LONG_CTX // 64)
    k0 = rng.standard_normal((nkv, LONG_CTX, d), dtype=np.float32)
    v0 = rng.standard_normal((nkv, LONG_CTX, d), dtype=np.float32)
    kc, vc = _dev(k0, dev), _dev(v0, dev)
    q = ops.rope_kv_append(_dev(qkv, dev), kc, vc, _dev(cos, dev), _dev(sin, dev), pos0, nq, nkv, table=_dev(perm, dev, torch.int32))
    c, s = cos[pos0:pos0 + n, None, :], sin[pos0:pos0 + n, None, :]
    qr = _rope64(qkv[:, :nq * d].reshape(n, nq, d), c, s).reshape(n, nq * d)
    kr = _rope64(qkv[:, nq * d:(nq + nkv) * d].reshape(n, nkv, d), c, s).transpose(1, 0, 2)
    vr = qkv[:, (nq + nkv) * d:].reshape(n, nkv, d).transpose(1, 0, 2)
    kg, vg = to_np(kc), to_np(vc)
    kb, vb = _from_pages(kg, perm), _from_pages(vg, perm)
    assert_close("roped q", to_np(q), qr, atol=5e-5)
    assert_close("k rows through the table", kb[:, pos0:pos0 + n], kr, atol=5e-5)
    assert_close("v rows through the table", vb[:, pos0:pos0 + n], vr, atol=0)
    rows = np.ones(LONG_CTX, bool)
    rows[[perm[p // 64] * 64 + p % 64 for p in range(pos0, pos0 + n)]] = False
    assert np.array_equal(kg[:, rows], k0[:, rows]) and np.array_equal(vg[:, rows], v0[:, rows]), "rows outside [4090, 4102) changed"


_FA_LONG = {}


def _fa_long_inputs(S):
    """q [S, 32 * 128] and K / V [8, LONG_CTX, 128] (NaN past the context) for S = Sq = Sk, generated once per S."""
    if S not in _FA_LONG:
        _FA_LONG.clear()
        rng = np.random.default_rng(S)
        q = rng.standard_normal((S, 32 * 128), dtype=np.float32)
        kc = rng.standard_normal((8, LONG_CTX, 128), dtype=np.float32)
        vc = rng.standard_normal((8, LONG_CTX, 128), dtype=np.float32)
        kc[:, S:] = np.nan
        vc[:, S:] = np.nan
        rows = {0, 15, 16, 31, 32, 63, 64, 4063, 4064, 4095, 4096, 4097}          # tile / half-tile edges, both sides of 4096
        rows |= set(range((S - 1) // 64 * 64, S))                          # the last 64-key tile: every 16- and 32-row tail
        rows |= set(rng.choice(S, 64, replace=False).tolist())
        _FA_LONG[S] = (q, kc, vc, np.array(sorted(r for r in rows if r < S)))
    return _FA_LONG[S]


@pytest.mark.parametrize("S", [4097, 4600])
@pytest.mark.parametrize("rows,xcd", [(16, 1), (32, 1), (32, 0)], ids=["rows16", "rows32", "rows32-plain-grid"])
def test_attention_flash_form_long_prompt(dev, S, rows, xcd):
    """k_attn_fa at the model's prompt limit: Sq = Sk = 4097 (one row past 4096: a lone row in the last 16 / 32-row block) and 4600
    (72 key tiles, the last one 56 keys), causal, 32 : 8 heads, d = 128, K / V in cache layout with NaN rows past the context; the
    16-row form, the 32-row form on the XCD-aware block order and on the plain grid.  fp64 reference on a fixed sample of query rows:
    the tile and half-tile edges, both sides of 4064 and 4096, the whole last 64 rows (every tail), 64 random rows.
    ops.attention passes no K / V tile images (kv_img), so the image-tile forms k_attn_fa<1, true, *> are covered by the engine-level
    prefill of tests/test_long_context_gpu.py, not here."""
    from vita_amd import _lib, ops
    nq, nkv, d = 32, 8, 128
    q, kc, vc, sample = _fa_long_inputs(S)
    out = torch.full((S, nq * d), float("nan"), dtype=torch.float32, device=dev)
    _lib.tune("attn_fa", 2)
    _lib.tune("attn_rows", rows)
    _lib.tune("attn_xcd", xcd)
    try:
        ops.attention(_dev(q, dev), _dev(kc, dev), _dev(vc, dev), out, B=1, Hq=nq, Hkv=nkv, Sq=S, Sk=S, d=d, ldq=nq * d, hsq=d, ldk=d,
                      hsk=LONG_CTX * d, ldv=d, hsv=LONG_CTX * d, ldo=nq * d, scale=d ** -0.5, causal=True, q_off=0, klen=S)
    finally:
        _lib.tune("attn_fa", 1)
        _lib.tune("attn_rows", 0)
        _lib.tune("attn_xcd", 1)
    got = to_np(out)
    assert np.isfinite(got).all(), "NaN / inf in the output (a row past the context reached a product, or a row was not written)"
    G, scale = nq // nkv, d ** -0.5
    ref = np.empty((sample.size, nq * d))
    K, V = kc[:, :S].astype(np.float64), vc[:, :S].astype(np.float64)
    vis = np.arange(S)[None, :] <= sample[:, None]
    for hq in range(nq):
        sc = np.where(vis, (q[sample, hq * d:(hq + 1) * d].astype(np.float64) @ K[hq // G].T) * scale, -np.inf)
        p = np.exp(sc - sc.max(-1, keepdims=True))
        ref[:, hq * d:(hq + 1) * d] = (p / p.sum(-1, keepdims=True)) @ V[hq // G]
    assert_close(f"flash form S={S} rows={rows} xcd={xcd} ({sample.size} sampled rows)", got[sample], ref, atol=ATTN_X3_ATOL)
