"""Thin torch-tensor front end over the C ABI.  torch is plumbing here (device memory, current
stream); every computation is a HIP kernel in libvita_hip.so.  All operators require CUDA
(ROCm) tensors and raise otherwise — there is deliberately no CPU path."""
import ctypes as C

import torch

from . import _lib
from ._lib import AttnArgs, GemmArgs, check

ACT = {None: 0, "none": 0, "gelu": 1, "relu": 2, "silu": 3}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.VitaHipError("vita_amd operators need GPU tensors (no CPU fallback)")


def _c(t, name="tensor"):
    """kernels index raw pointers: require a dense row-major tensor (rows may be strided views)."""
    if t is not None and t.ndim >= 1 and t.stride(-1) != 1 and t.shape[-1] != 1:
        raise ValueError(f"{name} must be contiguous along its last dimension (got strides {t.stride()})")
    return t


def _dense(t):
    return t if t.is_contiguous() else t.contiguous()


def _f32(t, name="tensor"):
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t


def _bf16(t, name="weight"):
    if t.dtype != torch.bfloat16:
        raise TypeError(f"{name} must be bfloat16, got {t.dtype}")
    return t


_SCRATCH = {}


def _scratch(device, nbytes):
    """per-device scratch for split-K partial sums (stream-ordered reuse: every GEMM here runs on the current stream)."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    t = _SCRATCH.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(nbytes, 64 << 20), dtype=torch.uint8, device=device)
        _SCRATCH[key] = t
    return t


def gemm(a, w, *, w_up=None, bias=None, act=None, scale=None, resid=None, out=None, a_rowidx=None, a_rows=None,
         segrow=None, seglen=None, m=None, c_rowidx=None, group_off=None, ngroups=0, w_group_stride=0, lda=None,
         ldc=None, ksplit=0, ln=None):
    """out[orow(m), :] = epilogue(A[arow(m, k)] @ w.T).  a: fp32 [rows, lda]; w: bf16 [N, K] (or [E, N, K] grouped).
    ksplit: 0 = the library may split K over more blocks for small launches (plain GEMMs), 1 = never, n = n-way.
    ln = (weight, bias or None, eps): also returns LayerNorm(out) — (out, ln_out) — from the same call (vh_gemm_ln)."""
    _dev(a, w, out)
    _f32(_c(a, "a"), "a"); _bf16(w, "w")
    if not w.is_contiguous():
        raise ValueError("w must be contiguous")
    lib = _lib.load()
    g = GemmArgs()
    N, K = int(w.shape[-2]), int(w.shape[-1])
    g.A = a.data_ptr(); g.lda = int(lda if lda is not None else a.stride(0))
    g.a_rows = int(a_rows if a_rows is not None else a.shape[0])
    g.a_rowidx = a_rowidx.data_ptr() if a_rowidx is not None else None
    if segrow is None:
        g.nseg, g.seglen = 1, K
        g.segrow[0] = 0
    else:
        g.nseg, g.seglen = len(segrow), int(seglen)
        for i, v in enumerate(segrow):
            g.segrow[i] = int(v)
    g.W = w.data_ptr(); g.W_up = w_up.data_ptr() if w_up is not None else None
    g.ldw = K; g.w_group_stride = int(w_group_stride)
    g.group_off = group_off.data_ptr() if group_off is not None else None
    g.ngroups = int(ngroups)
    M = int(m if m is not None else (a_rowidx.shape[0] if a_rowidx is not None else a.shape[0]))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    g.C = out.data_ptr(); g.ldc = int(ldc if ldc is not None else out.stride(0))
    g.c_rowidx = c_rowidx.data_ptr() if c_rowidx is not None else None
    g.bias = bias.data_ptr() if bias is not None else None
    g.scale = scale.data_ptr() if scale is not None else None
    if resid is not None:
        g.resid = resid.data_ptr(); g.ldr = int(resid.stride(0))
    g.M, g.N, g.K, g.act = M, N, K, ACT[act]
    g.ksplit = int(ksplit)
    if ksplit != 1 and group_off is None and w_up is None and c_rowidx is None and M * N <= (8 << 20):
        # room for up to 8 partial-sum slabs, capped at 96 MB (the library lowers the split to what fits)
        ws = _scratch(a.device, min(8 * 4 * M * N, 96 << 20))
        g.ws, g.ws_bytes = ws.data_ptr(), ws.numel()
    if ln is not None:
        lw, lb, eps = ln
        _dev(lw); _f32(_c(lw, "ln weight"), "ln weight")
        ln_out = torch.empty((M, N), dtype=torch.float32, device=a.device)
        check(lib.vh_gemm_ln(C.byref(g), _p(lw), _p(lb), float(eps), _p(ln_out), int(ln_out.stride(0)), _stream()), "vh_gemm_ln")
        return out, ln_out
    check(lib.vh_gemm(C.byref(g), _stream()), "vh_gemm")
    return out


def attention(q, k, v, out, *, B, Hq, Hkv, Sq, Sk, d, ldq, hsq, ldk, hsk, ldv, hsv, ldo, bsq=0, bsk=0, bso=0, scale,
              causal=False, q_off=0, klen=None, chunk=0, left=-1, p=None, ldp=0, hsp=0, bias_u=None, bias_v=None, klens=None):
    """klens: int32 device tensor [B], batch b masks keys >= klens[b] (the pad mask of a padded batch); klen must then be
    their maximum (None: Sk, always a valid bound)."""
    _dev(q, k, v, out, klens)
    for t, nm in ((q, "q"), (k, "k"), (v, "v"), (out, "out"), (p, "p")):
        _c(t, nm)
    lib = _lib.load()
    a = AttnArgs()
    a.Q, a.ldq, a.hsq = q.data_ptr(), ldq, hsq
    a.K, a.ldk, a.hsk = k.data_ptr(), ldk, hsk
    a.V, a.ldv, a.hsv = v.data_ptr(), ldv, hsv
    if p is not None:
        a.P, a.ldp, a.hsp = p.data_ptr(), ldp, hsp
        a.bias_u, a.bias_v = bias_u.data_ptr(), bias_v.data_ptr()
    a.O, a.ldo = out.data_ptr(), ldo
    a.bsq, a.bsk, a.bso = bsq, bsk, bso
    a.B, a.Hq, a.Hkv, a.Sq, a.Sk, a.d = B, Hq, Hkv, Sq, Sk, d
    a.causal, a.q_off = int(causal), q_off
    a.klen = Sk if klen is None else int(klen)
    a.chunk, a.left = int(chunk), int(left)
    a.scale = float(scale)
    a.klens = _klens(klens, B)
    check(lib.vh_attention(C.byref(a), _stream()), "vh_attention")
    return out


def _klens(klens, B):
    if klens is None:
        return None
    if klens.dtype != torch.int32 or klens.ndim != 1 or klens.shape[0] != B or not klens.is_contiguous():
        raise ValueError(f"klens must be a contiguous int32 tensor of {B} entries")
    return klens.data_ptr()


class EncoderScratch:
    """Caller-owned scratch of vh_encoder_layer for [M, C] rows and an MLP of width F (reused by every layer of a pass)."""

    def __init__(self, M, Cw, F, device):
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        self.M, self.C, self.F = M, Cw, F
        self.qkv, self.attn, self.hmid, self.mid = f(M, 3 * Cw), f(M, Cw), f(M, Cw), f(M, F)
        self.h = [f(M, Cw), f(M, Cw)]                       # LayerNorm outputs, ping-pong between layers
        self.ws = _scratch(device, min(8 * 4 * M * max(3 * Cw, F), 96 << 20))


_ENC_SCRATCH = {}
ENC_SCRATCH_CAP_BYTES = 768 << 20      # all cached sets together (an 8-tile ViT batch is ~370 MB, 13 tiles ~600 MB)


def _enc_scratch_bytes(sc):
    return 4 * sc.M * (3 * sc.C + 2 * sc.C + sc.F + 2 * sc.C)


def encoder_scratch(M, Cw, F, device):
    """EncoderScratch for (M, C, F), kept per (device, current stream) across passes: building it costs six allocations (~0.1 ms of host
    time in front of a tower pass, r04 trace); reuse is stream-ordered like _scratch.  At most four shapes and at most
    ENC_SCRATCH_CAP_BYTES in all are kept (dynamic tiling makes M vary per request, and four 13-tile sets would pin ~2 GB
    behind a KV pool that was sized from free memory); the key holds the torch Stream OBJECT, so its handle cannot be handed to
    another stream while an entry is alive."""
    stream = torch.cuda.current_stream(device)
    key = (device.type, device.index, stream, int(M), int(Cw), int(F))
    sc = _ENC_SCRATCH.pop(key, None)
    if sc is None:
        sc = EncoderScratch(M, Cw, F, device)
    _ENC_SCRATCH[key] = sc                                                  # most recently used last
    while len(_ENC_SCRATCH) > 1 and (len(_ENC_SCRATCH) > 4 or sum(_enc_scratch_bytes(v) for v in _ENC_SCRATCH.values()) > ENC_SCRATCH_CAP_BYTES):
        _ENC_SCRATCH.pop(next(iter(_ENC_SCRATCH)))                          # evict the least recently used; the current one stays
    sc.ws = _scratch(device, min(8 * 4 * M * max(3 * Cw, F), 96 << 20))     # (the shared split-K scratch may have been regrown)
    return sc


def encoder_layer(x, h_in, h_out, L, sc, *, heads, B, act, eps, next_norm=None, p=None, bias_u=None, bias_v=None, klen=-1, chunk=0,
                  left=-1, planes=False, klens=None):
    """One pre-norm transformer block in ONE library call (vh_encoder_layer): x [M, C] updated in place, h_in = LN(x; norm1),
    h_out = LN(x_out; next_norm) when next_norm = (w, b) is given.  L: dict of this layer's weights (qkv_w, qkv_b, proj_w,
    proj_b, ls1?, n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b, ls2?).  planes=True: h_in / h_out hold bf16 hi/lo planes (split_planes_into) in
    their M * C * 4 bytes and the Linears run on the weight-streaming GEMM (vita_hip.h: vh_encoder_layer_args.planes).
    klens: int32 device tensor [B] of per-sequence key lengths (klen = their maximum)."""
    _dev(x, h_in, klens)
    a = _lib.EncoderLayerArgs()
    a.x, a.h_in, a.h_out = x.data_ptr(), h_in.data_ptr(), (h_out.data_ptr() if next_norm is not None else None)
    a.M, a.C, a.F, a.heads, a.B = sc.M, sc.C, sc.F, int(heads), int(B)
    if tuple(x.shape) != (sc.M, sc.C) or not x.is_contiguous() or not h_in.is_contiguous():
        raise ValueError("encoder_layer: x / h_in must be contiguous [M, C] rows matching the scratch")
    a.qkv_w, a.qkv_b = L["qkv_w"].data_ptr(), L["qkv_b"].data_ptr()
    a.proj_w, a.proj_b, a.ls1 = L["proj_w"].data_ptr(), L["proj_b"].data_ptr(), _p(L.get("ls1"))
    a.n2_w, a.n2_b = L["n2w"].data_ptr(), L["n2b"].data_ptr()
    a.fc1_w, a.fc1_b = L["fc1_w"].data_ptr(), L["fc1_b"].data_ptr()
    a.fc2_w, a.fc2_b, a.ls2 = L["fc2_w"].data_ptr(), L["fc2_b"].data_ptr(), _p(L.get("ls2"))
    if next_norm is not None:
        a.next_w, a.next_b = next_norm[0].data_ptr(), _p(next_norm[1])
    a.act, a.eps = ACT[act], float(eps)
    if p is not None:
        a.P, a.ldp, a.bias_u, a.bias_v = p.data_ptr(), int(p.stride(0)), bias_u.data_ptr(), bias_v.data_ptr()
    a.klen, a.chunk, a.left = int(klen), int(chunk), int(left)
    a.qkv, a.attn, a.hmid, a.mid = sc.qkv.data_ptr(), sc.attn.data_ptr(), sc.hmid.data_ptr(), sc.mid.data_ptr()
    a.ws, a.ws_bytes = sc.ws.data_ptr(), sc.ws.numel() * sc.ws.element_size()
    a.planes = int(bool(planes))
    a.klens = _klens(klens, int(B))
    check(_lib.load().vh_encoder_layer(C.byref(a), _stream()), "vh_encoder_layer")


def layernorm(x, w, b, eps, *, act=None, post_scale=1.0, out=None):
    _dev(x, w)
    _c(x, "x")
    rows, cols = x.shape[0], x.shape[1]
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
    check(_lib.load().vh_layernorm(_p(x), x.stride(0), _p(out), out.stride(0), _p(w), _p(b), rows, cols, eps,
                                   ACT[act], post_scale, _stream()), "vh_layernorm")
    return out


def rmsnorm(x, w, eps, out=None):
    _dev(x, w)
    x = _dense(x)
    if out is None:
        out = torch.empty_like(x)
    check(_lib.load().vh_rmsnorm(_p(x), _p(out), _p(w), x.shape[0], x.shape[1], eps, _stream()), "vh_rmsnorm")
    return out


def hash_row_blocks(x, out=None):
    """128-bit content digests of the complete 64-row blocks of x fp32 [rows, cols] (rows may be strided) -> uint32 words as int32
    [rows // 64, 4] on the device (vh_hash_row_blocks; the definition is in include/vita_hip.h).  Enqueued on the current stream."""
    _dev(x)
    _f32(_c(x, "x"), "x")
    if x.ndim != 2:
        raise ValueError("hash_row_blocks takes a [rows, cols] tensor")
    rows, cols = x.shape
    if out is None:
        out = torch.empty((rows // 64, 4), dtype=torch.int32, device=x.device)
    elif out.dtype != torch.int32 or not out.is_contiguous() or out.numel() < (rows // 64) * 4:
        raise ValueError("out must be a contiguous int32 tensor of at least [rows // 64, 4]")
    check(_lib.load().vh_hash_row_blocks(_p(x), x.stride(0) if rows > 1 else cols, rows, cols, _p(out), _stream()), "vh_hash_row_blocks")
    return out


def vit_patchify(pix, patch, kpad):
    _dev(pix)
    pix = _dense(pix)
    n, _, img, _ = pix.shape
    g = img // patch
    out = torch.empty((n * g * g, kpad), dtype=torch.float32, device=pix.device)
    check(_lib.load().vh_vit_patchify(_p(pix), _p(out), n, img, patch, kpad, _stream()), "vh_vit_patchify")
    return out


def vit_embed(pix, patch, kpad, patch_w, patch_b, cls, pos, ln_w, ln_b, eps, ntok, x, h, h_planes=None):
    """InternVisionEmbeddings + the first block's norm1 in one library call (vh_vit_embed): pix [n,3,S,S] -> x [n*ntok, C] (residual
    stream), h = LayerNorm(x) fp32 and, when h_planes (any dense buffer of n*ntok*C*4 bytes) is given, its bf16 hi/lo planes."""
    _dev(pix, x, h)
    pix = _dense(pix)
    n, _, img, _ = pix.shape
    g = img // patch
    Cw = int(patch_w.shape[0])
    patches = torch.empty((n * g * g, kpad), dtype=torch.float32, device=pix.device)
    pe = torch.empty((n * g * g, Cw), dtype=torch.float32, device=pix.device)
    M = n * g * g
    ws = _scratch(pix.device, min(8 * 4 * M * Cw, 96 << 20))
    a = _lib.VitEmbedArgs()
    a.pix, a.n, a.img, a.patch, a.kpad = pix.data_ptr(), n, img, int(patch), int(kpad)
    a.patch_w, a.patch_b, a.cls, a.pos = patch_w.data_ptr(), patch_b.data_ptr(), cls.data_ptr(), pos.data_ptr()
    a.ln_w, a.ln_b, a.eps = ln_w.data_ptr(), _p(ln_b), float(eps)
    a.ntok, a.C = int(ntok), Cw
    a.patches, a.pe, a.x, a.h = patches.data_ptr(), pe.data_ptr(), x.data_ptr(), h.data_ptr()
    a.h_planes = h_planes.data_ptr() if h_planes is not None else None
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    check(_lib.load().vh_vit_embed(C.byref(a), _stream()), "vh_vit_embed")
    return x, h


def vit_assemble(patches, cls, pos, n, ntok, hid):
    x = torch.empty((n * ntok, hid), dtype=torch.float32, device=patches.device)
    check(_lib.load().vh_vit_assemble(_p(patches), _p(cls), _p(pos), _p(x), n, ntok, hid, _stream()),
          "vh_vit_assemble")
    return x


def vit_pixel_shuffle(x, n, grid, hid, mul):
    g2 = grid // 2
    out = torch.empty((n, g2 * g2, 4 * hid), dtype=torch.float32, device=x.device)
    check(_lib.load().vh_vit_pixel_shuffle(_p(x), _p(out), n, grid, hid, mul, _stream()), "vh_vit_pixel_shuffle")
    return out


def audio_conv1(feats, mean, istd, w, b):
    _dev(feats, w)
    feats = _dense(feats)
    T, F = feats.shape
    Cc = w.shape[0]
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    out = torch.empty((T1 * F1, Cc), dtype=torch.float32, device=feats.device)
    check(_lib.load().vh_audio_conv1(_p(feats), _p(mean), _p(istd), _p(w), _p(b), _p(out), T, F, Cc, _stream()),
          "vh_audio_conv1")
    return out, T1, F1


def audio_conv1_batch(feats, mean, istd, w, b):
    """vh_audio_conv1_batch: feats fp32 [B, T, F] (clips padded to a common T) -> ([B * T1 * F1, C], T1, F1), clip after clip."""
    _dev(feats, w)
    feats = _dense(_f32(feats, "feats"))
    Bn, T, F = feats.shape
    Cc = w.shape[0]
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    out = torch.empty((Bn * T1 * F1, Cc), dtype=torch.float32, device=feats.device)
    check(_lib.load().vh_audio_conv1_batch(_p(feats), _p(mean), _p(istd), _p(w), _p(b), _p(out), Bn, T, F, Cc, _stream()),
          "vh_audio_conv1_batch")
    return out, T1, F1


def audio_mask_rows(x, klens, B, gap):
    """vh_audio_mask_rows: x fp32 [B * S, cols] -> [B * (S + gap), cols] with rows >= klens[b] of clip b (and its gap rows) zero."""
    _dev(x, klens)
    _f32(_c(x, "x"), "x")
    if x.shape[0] % B:
        raise ValueError("audio_mask_rows: rows must be a multiple of B")
    Sn, cols = x.shape[0] // B, x.shape[1]
    out = torch.empty((B * (Sn + gap), cols), dtype=torch.float32, device=x.device)
    check(_lib.load().vh_audio_mask_rows(_p(x), x.stride(0), _p(out), out.stride(0), _klens(klens, B), B, Sn, int(gap), cols,
                                         _stream()), "vh_audio_mask_rows")
    return out


def embed_splice(kind, idx, embed, img, aud, H):
    S = kind.shape[0]
    out = torch.empty((S, H), dtype=torch.float32, device=embed.device)
    check(_lib.load().vh_embed_splice(_p(kind), _p(idx), _p(embed), _p(img), _p(aud), _p(out), S, H, _stream()),
          "vh_embed_splice")
    return out


def split_planes(x):
    """fp32 [rows, cols] -> (hi, lo) bf16 planes with x = hi + lo to 2^-17 (the pre-split GEMM operand)."""
    _dev(x)
    _f32(_c(x, "x"), "x")
    rows, cols = x.shape
    hi = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    lo = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    check(_lib.load().vh_split_planes(_p(x), x.stride(0), _p(hi), _p(lo), cols, rows, cols, _stream()),
          "vh_split_planes")
    return hi, lo


def split_planes_into(x, buf):
    """fp32 x [rows, cols] -> bf16 hi plane then lo plane inside `buf` (any dense tensor of rows * cols * 4 bytes): the operand layout of
    vh_encoder_layer's planes mode."""
    _dev(x, buf)
    _f32(_c(x, "x"), "x")
    rows, cols = x.shape
    if buf.numel() * buf.element_size() < rows * cols * 4 or not buf.is_contiguous():
        raise ValueError("split_planes_into: buf must be a dense tensor of at least rows * cols * 4 bytes")
    base = buf.data_ptr()
    check(_lib.load().vh_split_planes(_p(x), x.stride(0), base, base + rows * cols * 2, cols, rows, cols, _stream()), "vh_split_planes")
    return buf


def _gemm_ps_args(a_hi, a_lo, w, *, bias, act, scale, resid, out, out_split, a_rowidx, m, c_rowidx, group_off, ngroups,
                  w_group_stride, ksplit, nslab_out, out_planes):
    """vh_gemm_ps_args of gemm_ps / gemm_ps_i8 without the weight pointers -> (args, planes or None, out or None)."""
    g = _lib.GemmPsArgs()
    N, K = int(w.shape[-2]), int(w.shape[-1])
    g.A_hi, g.A_lo, g.lda = a_hi.data_ptr(), a_lo.data_ptr(), int(a_hi.stride(0))
    g.a_rowidx = a_rowidx.data_ptr() if a_rowidx is not None else None
    g.ldw, g.w_group_stride = int(w.stride(-2)), int(w_group_stride)
    g.group_off = group_off.data_ptr() if group_off is not None else None
    g.ngroups = int(ngroups)
    M = int(m if m is not None else (a_rowidx.shape[0] if a_rowidx is not None else a_hi.shape[0]))
    planes = None
    if out_split:
        if out_planes is not None:
            planes = tuple(out_planes)
            _dev(*planes)
            for t in planes:
                _bf16(_c(t, "out_planes"), "out_planes")
                if t.ndim != 2 or t.shape[0] < M or t.shape[1] != N:
                    raise ValueError(f"out_planes must be [>= {M}, {N}] bf16 views, got {tuple(t.shape)}")
            if planes[0].stride(0) != planes[1].stride(0):
                raise ValueError("out_planes: hi and lo need the same row stride")
        else:
            planes = (torch.empty((M, N), dtype=torch.bfloat16, device=w.device),
                      torch.empty((M, N), dtype=torch.bfloat16, device=w.device))
        g.C_hi, g.C_lo, g.ldc_split = planes[0].data_ptr(), planes[1].data_ptr(), int(planes[0].stride(0))
    if not out_split or out is not None:
        if out is None:
            out = torch.empty((M, N), dtype=torch.float32, device=w.device)
        if ksplit > 1 or ksplit < 0:
            if out.ndim != 3 or out.shape[0] != abs(ksplit):
                raise ValueError("ksplit > 1 needs out of shape [ksplit, rows, N] (ksplit < 0: [-ksplit, rows, N])")
            g.C, g.ldc, g.c_split_stride = out.data_ptr(), int(out.stride(1)), int(out.stride(0))
        else:
            g.C, g.ldc = out.data_ptr(), int(out.stride(0))
    g.ksplit = int(ksplit)
    g.nslab_out = nslab_out.data_ptr() if nslab_out is not None else None
    g.c_rowidx = c_rowidx.data_ptr() if c_rowidx is not None else None
    g.bias = bias.data_ptr() if bias is not None else None
    g.scale = scale.data_ptr() if scale is not None else None
    if resid is not None:
        g.resid, g.ldr = resid.data_ptr(), int(resid.stride(0))
    g.M, g.N, g.K, g.act = M, N, K, ACT[act]
    return g, planes, out


def gemm_ps(a_hi, a_lo, w, *, w_up=None, bias=None, act=None, scale=None, resid=None, out=None, out_split=False,
            a_rowidx=None, m=None, c_rowidx=None, group_off=None, ngroups=0, w_group_stride=0, wide=False, ksplit=1,
            nslab_out=None, out_planes=None):
    """Weight-streaming GEMM on pre-split activations (vh_gemm_ps).  Returns fp32 out, or (hi, lo) planes when
    out_split=True (out_planes: write them into these two bf16 [rows, N] views of equal row stride instead of new tensors).
    ksplit > 1: `out` must be [ksplit, rows, N] (partial sums per K range; the caller adds them)."""
    _dev(a_hi, a_lo, w)
    _bf16(a_hi, "a_hi"); _bf16(a_lo, "a_lo"); _bf16(w, "w")
    g, planes, out = _gemm_ps_args(a_hi, a_lo, w, bias=bias, act=act, scale=scale, resid=resid, out=None if out_split else out,
                                   out_split=out_split, a_rowidx=a_rowidx, m=m, c_rowidx=c_rowidx, group_off=group_off,
                                   ngroups=ngroups, w_group_stride=w_group_stride, ksplit=ksplit, nslab_out=nslab_out,
                                   out_planes=out_planes)
    g.W = w.data_ptr(); g.W_up = w_up.data_ptr() if w_up is not None else None
    g.ldw = int(w.shape[-1])
    g.wide = int(bool(wide))
    check(_lib.load().vh_gemm_ps(C.byref(g), _stream()), "vh_gemm_ps")
    return planes if out_split else out


def gemm_ps_i8(a_hi, a_lo, w, s, *, w_up=None, s_up=None, s_group_stride=0, bias=None, act=None, scale=None, resid=None, out=None,
               out_split=False, a_rowidx=None, m=None, c_rowidx=None, group_off=None, ngroups=0, w_group_stride=0, ksplit=1,
               nslab_out=None, out_planes=None):
    """gemm_ps on int8 weights (vh_gemm_ps_i8): w / w_up int8 [.., N, K] (rows contiguous; the row stride is taken from
    the tensor, so a column range of a wider matrix is a legal operand), s / s_up fp32 scales, column n of group e scaled by
    s[e * s_group_stride + n].  The keywords are gemm_ps's without `wide`; with out_split=True an fp32 `out` may be given as well
    (the kernel then writes C and the planes) and the result is (hi, lo)."""
    _dev(a_hi, a_lo, w, s, w_up, s_up)
    _bf16(a_hi, "a_hi"); _bf16(a_lo, "a_lo")
    for t, nm in ((w, "w"), (w_up, "w_up")):
        if t is not None and (t.dtype != torch.int8 or t.stride(-1) != 1):
            raise TypeError(f"{nm} must be int8 with contiguous rows, got {t.dtype} strides {t.stride()}")
    for t, nm in ((s, "s"), (s_up, "s_up")):
        if t is not None:
            _f32(t, nm)
    if (w_up is None) != (s_up is None):
        raise ValueError("w_up and s_up go together")
    if w_up is not None and (w_up.shape[-2:] != w.shape[-2:] or w_up.stride(-2) != w.stride(-2)):
        raise ValueError("w_up must have w's [N, K] and row stride")
    g, planes, out = _gemm_ps_args(a_hi, a_lo, w, bias=bias, act=act, scale=scale, resid=resid, out=out, out_split=out_split,
                                   a_rowidx=a_rowidx, m=m, c_rowidx=c_rowidx, group_off=group_off, ngroups=ngroups,
                                   w_group_stride=w_group_stride, ksplit=ksplit, nslab_out=nslab_out, out_planes=out_planes)
    check(_lib.load().vh_gemm_ps_i8(C.byref(g), _p(w), _p(s), _p(w_up), _p(s_up), int(s_group_stride), _stream()), "vh_gemm_ps_i8")
    return planes if out_split else out


def gemm_ps_mxfp4(a_hi, a_lo, w, s, *, w_up=None, s_up=None, bias=None, act=None, scale=None, resid=None, out=None, out_split=False,
                  a_rowidx=None, m=None, c_rowidx=None, group_off=None, ngroups=0, w_group_stride=0, ksplit=1, nslab_out=None,
                  out_planes=None):
    """gemm_ps on MXFP4 weights (vh_gemm_ps_mxfp4): w / w_up uint8 e2m1 codes [.., N, K / 2] (element k in byte k >> 1, low
    nibble for even k), s / s_up uint8 E8M0 scale bytes [.., N, K / 32].  The row strides are taken from the tensors (a column range
    of a wider matrix is a legal operand when the scales are the same range: s.stride(-2) * 16 == w.stride(-2)); w_group_stride
    counts WEIGHTS.  The keywords are gemm_ps's without `wide`."""
    _dev(a_hi, a_lo, w, s, w_up, s_up)
    _bf16(a_hi, "a_hi"); _bf16(a_lo, "a_lo")
    for t, nm in ((w, "w"), (w_up, "w_up"), (s, "s"), (s_up, "s_up")):
        if t is not None and (t.dtype != torch.uint8 or t.stride(-1) != 1):
            raise TypeError(f"{nm} must be uint8 with contiguous rows, got {t.dtype} strides {t.stride()}")
    for cw, cs, nm in ((w, s, "s"), (w_up, s_up, "s_up")):
        if (cw is None) != (cs is None):
            raise ValueError("w_up and s_up go together")
        if cw is not None and (cs.shape[-2] != cw.shape[-2] or cs.shape[-1] * 16 != cw.shape[-1] or cs.stride(-2) * 16 != cw.stride(-2)):
            raise ValueError(f"{nm} must be [.., N, K / 32] with 1 / 16 of the codes' row stride, got {tuple(cs.shape)} strides {cs.stride()}")
    g, planes, out = _gemm_ps_args(a_hi, a_lo, w, bias=bias, act=act, scale=scale, resid=resid, out=out, out_split=out_split,
                                   a_rowidx=a_rowidx, m=m, c_rowidx=c_rowidx, group_off=group_off, ngroups=ngroups,
                                   w_group_stride=w_group_stride, ksplit=ksplit, nslab_out=nslab_out, out_planes=out_planes)
    g.K, g.ldw = 2 * int(w.shape[-1]), 2 * int(w.stride(-2))          # counted in weights, two per code byte
    check(_lib.load().vh_gemm_ps_mxfp4(C.byref(g), _p(w), _p(s), _p(w_up), _p(s_up), _stream()), "vh_gemm_ps_mxfp4")
    return planes if out_split else out


# ---- batch-1 decode operators, one by one (include/vita_hip.h: "batch-1 decode operators") --------------------------------
def router_top2(x, wg, want_probs=False):
    """MixtralSparseMoeBlock's gate on normed rows x [rows, H] fp32, wg bf16 [E, H] -> (ids int32 [rows, 2], weights fp32
    [rows, 2][, softmax fp32 [rows, E]])."""
    _dev(x, wg)
    _f32(_c(x, "x"), "x"); _bf16(_c(wg, "wg"), "wg")
    rows, H = x.shape
    E = wg.shape[0]
    ids = torch.empty((rows, 2), dtype=torch.int32, device=x.device)
    wts = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    probs = torch.empty((rows, E), dtype=torch.float32, device=x.device) if want_probs else None
    check(_lib.load().vh_router_top2(_p(x), x.stride(0), _p(wg), E, H, rows, _p(ids), _p(wts), _p(probs), _stream()), "vh_router_top2")
    return (ids, wts, probs) if want_probs else (ids, wts)


def moe_decode(x, norm_w, eps, wg, w1, w3, w2, delta=None):
    """block_sparse_moe(post_attention_layernorm(x + delta)) for ONE token (no residual add): x fp32 [H], w1 / w3 bf16
    [E, I, H], w2 bf16 [E, H, I] -> (y fp32 [H], route int32 [4] = e0, e1, bits(w0), bits(w1))."""
    _dev(x, wg, w1, w3, w2)
    _f32(_c(x, "x"), "x")
    E, I, H = w1.shape
    y = torch.empty(H, dtype=torch.float32, device=x.device)
    route = torch.zeros(4, dtype=torch.int32, device=x.device)
    hbuf = torch.empty(2 * I, dtype=torch.float32, device=x.device)
    check(_lib.load().vh_moe_decode(_p(x), _p(delta), _p(norm_w), float(eps), _p(wg), _p(w1), _p(w3), _p(w2), E, I, H, None, _p(y),
                                    _p(route), _p(hbuf), _stream()), "vh_moe_decode")
    return y, route


def rope_kv_append(qkv, kcache, vcache, rope_cos, rope_sin, pos0, nq, nkv, table=None):
    """RoPE on q, k of S fused-QKV rows [S, (nq + 2 nkv) * 128] + KV append at [pos0, pos0 + S) -> q_roped fp32 [S, nq * 128];
    kcache / vcache fp32 [nkv, max_ctx, 128] are updated in place."""
    _dev(qkv, kcache, vcache)
    _f32(_c(qkv, "qkv"), "qkv")
    Sn = qkv.shape[0]
    q = torch.empty((Sn, nq * 128), dtype=torch.float32, device=qkv.device)
    check(_lib.load().vh_rope_kv_append(_p(qkv), qkv.stride(0), _p(q), _p(kcache), _p(vcache), _p(rope_cos), _p(rope_sin), Sn, int(pos0),
                                        nq, nkv, kcache.shape[1], _p(table), _stream()), "vh_rope_kv_append")
    return q


def attn_decode(qkv, kcache, vcache, pos, rope_cos, rope_sin, nq, nkv, scale, table=None):
    """one token's RoPE + KV append at `pos` + causal GQA attention over [0, pos] -> fp32 [nq * 128]."""
    _dev(qkv, kcache, vcache)
    max_ctx = kcache.shape[1]
    ns = (max_ctx + 63) // 64
    dev = qkv.device
    part_o = torch.empty((nq, ns, 128), dtype=torch.float32, device=dev)
    part_ml = torch.empty((nq, ns, 2), dtype=torch.float32, device=dev)
    tickets = torch.zeros(nkv, dtype=torch.int32, device=dev)
    out = torch.empty(nq * 128, dtype=torch.float32, device=dev)
    check(_lib.load().vh_attn_decode(_p(qkv), _p(kcache), _p(vcache), int(pos), _p(rope_cos), _p(rope_sin), nq, nkv, max_ctx, float(scale),
                                     _p(table), _p(part_o), _p(part_ml), _p(tickets), _p(out), _stream()), "vh_attn_decode")
    return out


def attn_decode_scratch(n, nq, nkv, max_ctx, device):
    """scratch and outputs of attn_decode_batch for n sequences: per sequence (part_o, part_ml, tickets (zeroed), attn_out)."""
    ns = (max_ctx + 63) // 64
    return [(torch.empty((nq, ns, 128), dtype=torch.float32, device=device), torch.empty((nq, ns, 2), dtype=torch.float32, device=device),
             torch.zeros(nkv, dtype=torch.int32, device=device), torch.empty(nq * 128, dtype=torch.float32, device=device))
            for _ in range(n)]


def attn_decode_batch(qkvs, kcache, vcache, positions, rope_cos, rope_sin, nq, nkv, scale, tables, scratch=None):
    """attn_decode for up to 4 sequences of one paged pool in ONE launch (vh_attn_decode_batch, the batched decode iteration's
    attention kernel): sequence b appends qkvs[b] at positions[b] through its page table tables[b] (int32, disjoint pages) and
    attends over [0, positions[b]] -> list of fp32 [nq * 128] (the attn_out tensors of `scratch`, default: fresh
    attn_decode_scratch buffers; tickets must be zero before the first call and are left zero)."""
    _dev(kcache, vcache, *qkvs)
    n, max_ctx = len(qkvs), kcache.shape[1]
    if not (n == len(positions) == len(tables)) or (scratch is not None and len(scratch) != n):
        raise ValueError("attn_decode_batch: one position, page table and scratch entry per sequence")
    for q in qkvs:
        _f32(_c(q, "qkv"), "qkv")
    if scratch is None:
        scratch = attn_decode_scratch(n, nq, nkv, max_ctx, kcache.device)

    def ptrs(ts):
        return (C.c_void_p * max(n, 1))(*[None if t is None else t.data_ptr() for t in ts])
    pos =(C.c_int * max(n, 1))(*[int(p) for p in positions])
    check(_lib.load().vh_attn_decode_batch(n, ptrs(qkvs), _p(kcache), _p(vcache), pos, _p(rope_cos), _p(rope_sin), nq, nkv, max_ctx,
                                           float(scale), ptrs(tables), ptrs([s[0] for s in scratch]), ptrs([s[1] for s in scratch]),
                                           ptrs([s[2] for s in scratch]), ptrs([s[3] for s in scratch]), _stream()),
          "vh_attn_decode_batch")
    return [s[3] for s in scratch]


def attn_rows_scratch(n, nq, max_klen, device):
    """scratch of attn_rows that holds n rows of up to max_klen keys in one launch pair (uint8, vh_attn_rows_scratch_bytes)."""
    nbytes = _lib.load().vh_attn_rows_scratch_bytes(int(n), int(nq), int(max_klen))
    if nbytes == 0:
        raise ValueError("attn_rows_scratch: n, nq and max_klen must be positive")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def attn_rows(q, kcache, vcache, klens, tables, nq, nkv, scale, scratch=None, planes=False):
    """causal GQA attention of single query rows with q ALREADY rotated (vh_attn_rows, the decode rows of a mixed pass): row i of
    q [n, nq * 128] fp32 attends over keys [0, klens[i]) of the paged sequence tables[i] (int32 page table on the device) in the
    pools kcache / vcache fp32 [nkv, max_ctx, 128]; nothing is appended.  -> fp32 [n, nq * 128], or with planes=True the bf16
    (hi, lo) planes [n, nq * 128] whose sum is that row (what the O-projection GEMM reads)."""
    _dev(q, kcache, vcache)
    _f32(q, "q")
    n, max_ctx = q.shape[0], kcache.shape[1]
    if q.dim() != 2 or q.stride(1) != 1 or not (n == len(klens) == len(tables)):
        raise ValueError("attn_rows: q [n, nq * 128] with unit column stride, one key count and page table per row")
    if scratch is None:
        scratch = attn_rows_scratch(n, nq, max(int(k) for k in klens), q.device)
    kl = (C.c_int * max(n, 1))(*[int(k) for k in klens])
    tb = (C.c_void_p * max(n, 1))(*[None if t is None else t.data_ptr() for t in tables])
    if planes:
        hi = torch.empty((n, nq * 128), dtype=torch.bfloat16, device=q.device)
        lo = torch.empty_like(hi)
        out = None
    else:
        out = torch.empty((n, nq * 128), dtype=torch.float32, device=q.device)
        hi = lo = None
    check(_lib.load().vh_attn_rows(n, _p(q), q.stride(0), _p(kcache), _p(vcache), kl, tb, nq, nkv, max_ctx, float(scale), _p(scratch),
                                   scratch.numel() * scratch.element_size(), _p(out), _p(hi), _p(lo), nq * 128, _stream()), "vh_attn_rows")
    return (hi, lo) if planes else out


def lmhead_argmax(x, norm_w, eps, w, delta=None, nblk=1024):
    """logits = lm_head(rmsnorm(x + delta)) fp32 [V] and their argmax (int32 [1], lowest index on ties)."""
    _dev(x, w)
    V, H = w.shape
    logits = torch.empty(V, dtype=torch.float32, device=x.device)
    tok = torch.zeros(1, dtype=torch.int32, device=x.device)
    bv = torch.empty(nblk, dtype=torch.float32, device=x.device)
    bi = torch.empty(nblk, dtype=torch.int32, device=x.device)
    check(_lib.load().vh_lmhead_argmax(_p(x), _p(delta), _p(norm_w), float(eps), _p(w), V, H, _p(logits), _p(tok), _p(bv), _p(bi), nblk,
                                       _stream()), "vh_lmhead_argmax")
    return logits, tok


def sample_rows(logits, rows=None, temperature=1.0, top_k=0, top_p=1.0, seed=0, draw0=0):
    """Seeded draws (vh_sample_rows, the engine's device code): token r of `rows` is sampled from row r of logits fp32 [R, V]
    at draw index draw0 + r; a 1-D logits row is broadcast to `rows` draws.  -> int32 [rows]."""
    _dev(logits)
    if logits.dtype != torch.float32:
        raise TypeError("logits must be float32")
    if logits.dim() == 1:
        ld, V, n = 0, logits.shape[0], int(rows if rows is not None else 1)
    else:
        if logits.stride(1) != 1:
            raise ValueError("logits rows must be contiguous")
        ld, V, n = logits.stride(0), logits.shape[1], int(rows if rows is not None else logits.shape[0])
        if n > logits.shape[0]:
            raise ValueError("rows exceeds the logits rows")
    tok = torch.empty(n, dtype=torch.int32, device=logits.device)
    s = _lib.sampling(temperature, top_k, top_p, seed, draw0)
    check(_lib.load().vh_sample_rows(_p(logits), ld, n, V, C.byref(s), _p(tok), _stream()), "vh_sample_rows")
    return tok


def logit_rules_rows(logits, seen=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, tokens=None, logprobs=-1,
                     want_penalised=True):
    """The engine's logit rules (vh_logit_rules_rows) on rows of logits fp32 [R, V]: -> (penalised [R, V] or None, lp_tok [R] or
    None, lp_top_id [R, K] or None, lp_top [R, K] or None).  seen: int32 / uint32 [V] token table shared by the rows (bit 31 = in
    the prompt, low bits = output count; None = no history); tokens int32 [R] + logprobs = K >= 0: the log-probability of tokens[r]
    and the top K of the RAW row r."""
    _dev(logits)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise TypeError("logits must be float32 [R, V] with contiguous rows")
    R, V = logits.shape
    K = -1 if logprobs is None else int(logprobs)
    if seen is not None and (seen.numel() != V or seen.element_size() != 4 or not seen.is_contiguous()):
        raise ValueError("seen must be a contiguous 32-bit table of V entries")
    pen = torch.empty((R, V), dtype=torch.float32, device=logits.device) if want_penalised else None
    lp_tok = lp_id = lp_top = None
    if K >= 0:
        if tokens is None or tokens.dtype != torch.int32 or tokens.numel() != R:
            raise ValueError("logprobs need tokens int32 [R]")
        lp_tok = torch.empty(R, dtype=torch.float32, device=logits.device)
        lp_id = torch.empty((R, max(K, 1)), dtype=torch.int32, device=logits.device)
        lp_top = torch.empty((R, max(K, 1)), dtype=torch.float32, device=logits.device)
    r = _lib.logit_rules(repetition_penalty, presence_penalty, frequency_penalty, -1)
    check(_lib.load().vh_logit_rules_rows(_p(logits), logits.stride(0), R, V, C.byref(r), _p(seen) if seen is not None else None,
                                          _p(pen) if pen is not None else None, _p(tokens) if K >= 0 else None,
                                          _p(lp_tok) if K >= 0 else None, _p(lp_id) if K >= 0 else None,
                                          _p(lp_top) if K >= 0 else None, max(K, 0), _stream()), "vh_logit_rules_rows")
    if K >= 0:
        lp_id, lp_top = lp_id[:, :K], lp_top[:, :K]
    return pen, lp_tok, lp_id, lp_top

