// vh_api.hip — the C ABI (include/vita_hip.h): argument checking, error reporting, and the
// Mixtral engine that owns the layer loop for prefill and greedy decode so that one host call
// enqueues a whole forward (HF MixtralModel.forward + GenerationMixin greedy loop, as driven
// by vita/model/language_model/vita_mixtral.py:101-215 and video_audio_demo.py:257-270).
#include <dlfcn.h>
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../include/vita_hip.h"
#include "vh_kernels.h"

namespace {
thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
int check_launch(const char* what, int rc) {
    if (rc != 0) return fail(VH_E_SHAPE, "%s: unsupported shape/arguments", what);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VH_E_HIP, "%s: %s", what, hipGetErrorString(e));
    return VH_OK;
}
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
VhTuning g_tuning;
}  // namespace

VhTuning* vh_tuning() { return &g_tuning; }

extern "C" {

int vh_version(void) { return 100; }
const char* vh_last_error(void) { return g_err; }

int vh_tune(const char* key, int value) {
    if (!key) return fail(VH_E_ARG, "vh_tune: null key");
    if (!strcmp(key, "batch_moe_min")) { g_tuning.batch_moe_min = value; return VH_OK; }
    if (!strcmp(key, "batch_decode")) { g_tuning.batch_decode = value; return VH_OK; }
    if (!strcmp(key, "attn_impl")) { g_tuning.attn_impl = value; return VH_OK; }
    if (!strcmp(key, "attn_fa")) { g_tuning.attn_fa = value; return VH_OK; }
    if (!strcmp(key, "attn_rows")) { g_tuning.attn_rows = value; return VH_OK; }
    if (!strcmp(key, "step_attn")) { g_tuning.step_attn = value; return VH_OK; }
    if (!strcmp(key, "attn_ksplit")) { g_tuning.attn_ksplit = value; return VH_OK; }
    if (!strcmp(key, "prefill_attn_gemm")) { g_tuning.prefill_attn_gemm = value; return VH_OK; }
    if (!strcmp(key, "prefill_fuse_rows")) { g_tuning.prefill_fuse_rows = value; return VH_OK; }
    if (!strcmp(key, "ps_cfg")) { g_tuning.ps_cfg = value; return VH_OK; }
    if (!strcmp(key, "ps_nt")) { g_tuning.ps_nt = value; return VH_OK; }
    if (!strcmp(key, "ps_xcd")) { g_tuning.ps_xcd = value; return VH_OK; }
    if (!strcmp(key, "tp_overlap")) { g_tuning.tp_overlap = value; return VH_OK; }
    if (!strcmp(key, "moe_ksplit")) { g_tuning.moe_ksplit = value; return VH_OK; }
    if (!strcmp(key, "force_allreduce")) { g_tuning.force_allreduce = value; return VH_OK; }
    if (!strcmp(key, "tp_fuse")) { g_tuning.tp_fuse = value; return VH_OK; }
    if (!strcmp(key, "comm_allow_coarse")) { g_tuning.comm_allow_coarse = value; return VH_OK; }
    if (!strcmp(key, "comm_ranks_per_device")) { g_tuning.comm_ranks_per_device = value; return VH_OK; }
    if (!strcmp(key, "dec_fused")) { g_tuning.dec_fused = value; return VH_OK; }
    if (!strcmp(key, "dec_gateup_grid")) { g_tuning.dec_gateup_grid = value; return VH_OK; }
    if (!strcmp(key, "attn_img")) { g_tuning.attn_img = value; return VH_OK; }
    if (!strcmp(key, "attn_xcd")) { g_tuning.attn_xcd = value; return VH_OK; }
    return fail(VH_E_ARG, "vh_tune: unknown key '%s'", key);
}

static int gemm_entry(const char* name, const vh_gemm_args* a, const float* ln_w, const float* ln_b, float ln_eps, float* ln_out,
                      long ld_ln, void* stream);
int vh_gemm(const vh_gemm_args* a, void* stream) { return gemm_entry("vh_gemm", a, nullptr, nullptr, 0.f, nullptr, 0, stream); }
int vh_gemm_ln(const vh_gemm_args* a, const float* ln_w, const float* ln_b, float ln_eps, float* ln_out, long ld_ln, void* stream) {
    if (!ln_w || !ln_out) return fail(VH_E_ARG, "vh_gemm_ln: null pointer");
    return gemm_entry("vh_gemm_ln", a, ln_w, ln_b, ln_eps, ln_out, ld_ln, stream);
}
static int gemm_entry(const char* name, const vh_gemm_args* a, const float* ln_w, const float* ln_b, float ln_eps, float* ln_out,
                      long ld_ln, void* stream) {
    if (!a || !a->A || !a->W || !a->C) return fail(VH_E_ARG, "%s: null pointer", name);
    VhGemmArgs g{};
    g.ln_w = ln_w; g.ln_b = ln_b; g.ln_eps = ln_eps; g.ln_out = ln_out; g.ld_ln = ld_ln;
    g.A = a->A; g.lda = a->lda; g.a_rows = a->a_rows; g.a_rowidx = a->a_rowidx;
    g.nseg = a->nseg; g.seglen = a->seglen;
    for (int i = 0; i < 16; ++i) g.segrow[i] = a->segrow[i];
    g.W = a->W; g.W_up = a->W_up; g.ldw = a->ldw; g.w_group_stride = a->w_group_stride;
    g.group_off = a->group_off; g.ngroups = a->ngroups;
    g.C = a->C; g.ldc = a->ldc; g.c_rowidx = a->c_rowidx;
    g.bias = a->bias; g.scale = a->scale; g.resid = a->resid; g.ldr = a->ldr;
    g.M = a->M; g.N = a->N; g.K = a->K; g.act = a->act;
    g.ws = a->ws; g.ws_bytes = a->ws_bytes; g.ksplit = a->ksplit;
    if ((a->lda % 4) != 0 || (a->ldw % 8) != 0) return fail(VH_E_SHAPE, "%s: lda%%4 / ldw%%8 alignment", name);
    return check_launch(name, vhk_gemm(S(stream), g));
}

// the C ABI's vh_gemm_ps_args as the launchers' record (the quantised entries have checked that a->W / W_up are null)
static int ps_args(const char* name, const vh_gemm_ps_args* a, VhGemmPsArgs& g) {
    g.A_hi = a->A_hi; g.A_lo = a->A_lo; g.lda = a->lda; g.a_rowidx = a->a_rowidx;
    g.W = a->W; g.W_up = a->W_up; g.ldw = a->ldw; g.w_group_stride = a->w_group_stride;
    g.group_off = a->group_off; g.ngroups = a->ngroups;
    g.C = a->C; g.ldc = a->ldc; g.C_hi = a->C_hi; g.C_lo = a->C_lo; g.ldc_split = a->ldc_split;
    g.c_rowidx = a->c_rowidx; g.bias = a->bias; g.scale = a->scale; g.resid = a->resid; g.ldr = a->ldr;
    g.M = a->M; g.N = a->N; g.K = a->K; g.act = a->act;
    g.ksplit = a->ksplit; g.c_split_stride = a->c_split_stride; g.nslab_out = a->nslab_out;
    if ((size_t)a->lda * 2 * (size_t)(a->M > 0 ? a->M : 1) >= (1ull << 32))
        return fail(VH_E_SHAPE, "%s: activation plane above the 32-bit offset range", name);
    return VH_OK;
}
int vh_gemm_ps(const vh_gemm_ps_args* a, void* stream) {
    if (!a || !a->A_hi || !a->A_lo || !a->W) return fail(VH_E_ARG, "vh_gemm_ps: null pointer");
    VhGemmPsArgs g{};
    if (int rc = ps_args("vh_gemm_ps", a, g)) return rc;
    return check_launch("vh_gemm_ps", vhk_gemm_ps(S(stream), g));
}
int vh_gemm_ps_i8(const vh_gemm_ps_args* a, const int8_t* W, const float* s, const int8_t* W_up, const float* s_up,
                  long s_group_stride, void* stream) {
    if (!a || !a->A_hi || !a->A_lo || !W || !s || (W_up != nullptr) != (s_up != nullptr)) return fail(VH_E_ARG, "vh_gemm_ps_i8: null pointer");
    if (a->W || a->W_up) return fail(VH_E_ARG, "vh_gemm_ps_i8: args->W / W_up must be null (the weights are the int8 arguments)");
    VhGemmPsArgs g{};
    if (int rc = ps_args("vh_gemm_ps_i8", a, g)) return rc;
    const VhPsI8 q{W, W_up, s, s_up, s_group_stride};
    if (const char* why = vhk_gemm_ps_i8_refusal(g, q)) return fail(VH_E_SHAPE, "vh_gemm_ps_i8: %s", why);
    return check_launch("vh_gemm_ps_i8", vhk_gemm_ps_i8(S(stream), g, q));
}
int vh_quant_rows_i8(const uint16_t* w, long rows, int cols, long ld_src, int col0, int ncols, int8_t* q, long ld_dst, float* s,
                     void* stream) {
    if (!w || !q || !s) return fail(VH_E_ARG, "vh_quant_rows_i8: null pointer");
    return check_launch("vh_quant_rows_i8", vhk_quant_rows_i8(S(stream), w, rows, cols, ld_src, col0, ncols, q, ld_dst, s));
}
int vh_gemm_ps_mxfp4(const vh_gemm_ps_args* a, const uint8_t* W, const uint8_t* Sc, const uint8_t* W_up, const uint8_t* Sc_up, void* stream) {
    if (!a || !a->A_hi || !a->A_lo || !W || !Sc || (W_up != nullptr) != (Sc_up != nullptr)) return fail(VH_E_ARG, "vh_gemm_ps_mxfp4: null pointer");
    if (a->W || a->W_up) return fail(VH_E_ARG, "vh_gemm_ps_mxfp4: args->W / W_up must be null (the weights are the MXFP4 arguments)");
    VhGemmPsArgs g{};
    if (int rc = ps_args("vh_gemm_ps_mxfp4", a, g)) return rc;
    const VhPsF4 q{W, W_up, Sc, Sc_up};
    if (const char* why = vhk_gemm_ps_mxfp4_refusal(g, q)) return fail(VH_E_SHAPE, "vh_gemm_ps_mxfp4: %s", why);
    return check_launch("vh_gemm_ps_mxfp4", vhk_gemm_ps_mxfp4(S(stream), g, q));
}
int vh_quant_mxfp4(const uint16_t* w, long rows, int cols, long ld_src, int col0, int ncols, uint8_t* codes, long ld_codes_bytes,
                   uint8_t* scales, long ld_scales, void* stream) {
    if (!w || !codes || !scales) return fail(VH_E_ARG, "vh_quant_mxfp4: null pointer");
    return check_launch("vh_quant_mxfp4", vhk_quant_mxfp4(S(stream), w, rows, cols, ld_src, col0, ncols, codes, ld_codes_bytes, scales, ld_scales));
}
int vh_split_planes(const float* x, long ldx, uint16_t* hi, uint16_t* lo, long ldo, int rows, int cols, void* stream) {
    if (!x || !hi || !lo) return fail(VH_E_ARG, "vh_split_planes: null pointer");
    return check_launch("vh_split_planes", vhk_split_planes(S(stream), x, ldx, hi, lo, ldo, rows, cols));
}

int vh_attention(const vh_attn_args* a, void* stream) {
    if (!a || !a->Q || !a->K || !a->V || !a->O) return fail(VH_E_ARG, "vh_attention: null pointer");
    VhAttnArgs g{};
    g.Q = a->Q; g.ldq = a->ldq; g.hsq = a->hsq; g.K = a->K; g.ldk = a->ldk; g.hsk = a->hsk;
    g.V = a->V; g.ldv = a->ldv; g.hsv = a->hsv; g.P = a->P; g.ldp = a->ldp; g.hsp = a->hsp;
    g.bias_u = a->bias_u; g.bias_v = a->bias_v; g.O = a->O; g.ldo = a->ldo;
    g.bsq = a->bsq; g.bsk = a->bsk; g.bso = a->bso;
    g.B = a->B; g.Hq = a->Hq; g.Hkv = a->Hkv; g.Sq = a->Sq; g.Sk = a->Sk; g.d = a->d;
    g.causal = a->causal; g.q_off = a->q_off; g.klen = a->klen; g.chunk = a->chunk; g.left = a->left;
    g.scale = a->scale; g.klens = a->klens;
    if (a->P && (!a->bias_u || !a->bias_v)) return fail(VH_E_ARG, "vh_attention: rel-pos needs bias_u/bias_v");
    if ((a->ldk % 4) || (a->ldv % 4) || (a->hsk % 4) || (a->hsv % 4) || (a->bsk % 4) ||
        (reinterpret_cast<uintptr_t>(a->K) & 15) || (reinterpret_cast<uintptr_t>(a->V) & 15) ||
        (a->P && ((a->ldp % 4) || (a->hsp % 4) || (reinterpret_cast<uintptr_t>(a->P) & 15))))
        return fail(VH_E_SHAPE, "vh_attention: K/V/P rows must be 16-byte aligned (strides multiples of 4 floats)");
    if ((a->ldq % 4) || (a->hsq % 4) || (a->bsq % 4) || (a->ldo % 4) || (a->bso % 4) || (reinterpret_cast<uintptr_t>(a->Q) & 15) ||
        (reinterpret_cast<uintptr_t>(a->O) & 15) || (a->d != 64 && a->d != 128) || (a->P && a->d != 64))
        return fail(VH_E_SHAPE, "vh_attention: Q/O rows must be 16-byte aligned, head_dim 64 or 128 (rel-pos: 64)");
    const int rc = vhk_attn(S(stream), g);
    if (rc == -2) return fail(VH_E_ARG, "vh_attention: klens is honoured by the fp32 direct kernel only (rel-pos, a chunk mask or attn_impl 2; not causal, not paged)");
    return check_launch("vh_attention", rc);
}

int vh_layernorm(const float* x, long ldx, float* y, long ldy, const float* w, const float* b, int rows, int cols,
                 float eps, int act, float post_scale, void* stream) {
    return check_launch("vh_layernorm", vhk_layernorm(S(stream), x, ldx, y, ldy, w, b, rows, cols, eps, act, post_scale));
}
int vh_rmsnorm(const float* x, float* y, const float* w, int rows, int cols, float eps, void* stream) {
    return check_launch("vh_rmsnorm", vhk_rmsnorm(S(stream), x, y, w, rows, cols, eps));
}
int vh_add(float* x, const float* y, long n, void* stream) { return check_launch("vh_add", vhk_add(S(stream), x, y, n)); }
int vh_hash_row_blocks(const float* x, long ldx, int rows, int cols, uint32_t* out, void* stream) {
    if (rows < 0 || cols < 1 || ldx < cols) return fail(VH_E_ARG, "vh_hash_row_blocks: rows %d, cols %d, ldx %ld", rows, cols, ldx);
    if (rows < 64) return VH_OK;                 // no complete block: nothing is written
    if (!x || !out) return fail(VH_E_ARG, "vh_hash_row_blocks: null pointer");
    return check_launch("vh_hash_row_blocks", vhk_hash_row_blocks(S(stream), x, ldx, rows, cols, out));
}
int vh_cast_bf16_f32(const uint16_t* in, float* out, long n, void* stream) {
    return check_launch("vh_cast_bf16_f32", vhk_cast_bf16_f32(S(stream), in, out, n));
}
int vh_fill_hash_bf16(uint16_t* dst, long rows, long cols, long ld_dst, long ld_src, long idx0, uint64_t seed, void* stream) {
    if (!dst) return fail(VH_E_ARG, "vh_fill_hash_bf16: null pointer");
    return check_launch("vh_fill_hash_bf16", vhk_fill_hash_bf16(S(stream), dst, rows, cols, ld_dst, ld_src, idx0, seed));
}
int vh_vit_embed(const vh_vit_embed_args* a, void* stream) {
    if (!a || !a->pix || !a->patch_w || !a->cls || !a->pos || !a->ln_w || !a->patches || !a->pe || !a->x || !a->h)
        return fail(VH_E_ARG, "vh_vit_embed: null pointer");
    if (a->n < 1 || a->patch < 1 || a->img % a->patch != 0 || a->kpad % 64 != 0 || a->kpad < 3 * a->patch * a->patch || a->C % 8 != 0)
        return fail(VH_E_SHAPE, "vh_vit_embed: n %d img %d patch %d kpad %d C %d", a->n, a->img, a->patch, a->kpad, a->C);
    const int g = a->img / a->patch, rows = a->n * g * g, M = a->n * a->ntok;
    if (a->ntok != g * g + 1) return fail(VH_E_SHAPE, "vh_vit_embed: ntok %d is not grid^2 + 1 (%d)", a->ntok, g * g + 1);
    hipStream_t st = S(stream);
    int rc = check_launch("vh_vit_embed (patchify)", vhk_vit_patchify(st, a->pix, a->patches, a->n, a->img, a->patch, a->kpad));
    if (rc != VH_OK) return rc;
    VhGemmArgs gm{};
    gm.A = a->patches; gm.lda = a->kpad; gm.a_rows = rows; gm.nseg = 1; gm.seglen = a->kpad;
    gm.W = a->patch_w; gm.ldw = a->kpad; gm.C = a->pe; gm.ldc = a->C; gm.M = rows; gm.N = a->C; gm.K = a->kpad;
    gm.bias = a->patch_b; gm.ws = a->ws; gm.ws_bytes = a->ws_bytes; gm.ksplit = a->ws ? 0 : 1;
    if ((rc = check_launch("vh_vit_embed (patch Linear)", vhk_gemm(st, gm))) != VH_OK) return rc;
    if ((rc = check_launch("vh_vit_embed (assemble)", vhk_vit_assemble(st, a->pe, a->cls, a->pos, a->x, a->n, a->ntok, a->C))) != VH_OK) return rc;
    if ((rc = check_launch("vh_vit_embed (norm1)", vhk_layernorm(st, a->x, a->C, a->h, a->C, a->ln_w, a->ln_b, M, a->C, a->eps, VH_ACT_NONE, 1.0f))) != VH_OK)
        return rc;
    if (a->h_planes) {
        uint16_t* hi = reinterpret_cast<uint16_t*>(a->h_planes);
        rc = check_launch("vh_vit_embed (planes)", vhk_split_planes(st, a->h, a->C, hi, hi + (size_t)M * a->C, a->C, M, a->C));
    }
    return rc;
}

int vh_vit_patchify(const float* pix, float* out, int n, int img, int patch, int kpad, void* stream) {
    return check_launch("vh_vit_patchify", vhk_vit_patchify(S(stream), pix, out, n, img, patch, kpad));
}
int vh_vit_assemble(const float* patches, const uint16_t* cls, const uint16_t* pos, float* x, int n, int ntok,
                    int hid, void* stream) {
    return check_launch("vh_vit_assemble", vhk_vit_assemble(S(stream), patches, cls, pos, x, n, ntok, hid));
}
int vh_vit_pixel_shuffle(const float* x, float* out, int n, int grid, int hid, float mul, void* stream) {
    return check_launch("vh_vit_pixel_shuffle", vhk_vit_pixel_shuffle(S(stream), x, out, n, grid, hid, mul));
}
int vh_audio_conv1(const float* feats, const float* mean, const float* istd, const uint16_t* w, const float* b,
                   float* out, int T, int F, int C, void* stream) {
    return check_launch("vh_audio_conv1", vhk_audio_conv1(S(stream), feats, mean, istd, w, b, out, 1, T, F, C));
}
int vh_audio_conv1_batch(const float* feats, const float* mean, const float* istd, const uint16_t* w, const float* b,
                         float* out, int B, int T, int F, int C, void* stream) {
    if (!feats || !mean || !istd || !w || !b || !out) return fail(VH_E_ARG, "vh_audio_conv1_batch: null pointer");
    return check_launch("vh_audio_conv1_batch", vhk_audio_conv1(S(stream), feats, mean, istd, w, b, out, B, T, F, C));
}
int vh_audio_mask_rows(const float* x, long ldx, float* y, long ldy, const int* klens, int B, int Sn, int gap, int cols,
                       void* stream) {
    if (!x || !y || !klens) return fail(VH_E_ARG, "vh_audio_mask_rows: null pointer");
    return check_launch("vh_audio_mask_rows", vhk_audio_mask_rows(S(stream), x, ldx, y, ldy, klens, B, Sn, gap, cols));
}
int vh_embed_splice(const int* src_kind, const int* src_idx, const uint16_t* embed, const float* img_feats,
                    const float* aud_feats, float* out, int Sn, int H, void* stream) {
    return check_launch("vh_embed_splice",
                        vhk_embed_splice(S(stream), src_kind, src_idx, embed, img_feats, aud_feats, out, Sn, H));
}

// ---- batch-1 decode operators, one by one ("one entry per kernel K1-K28 group") ----------------------------
// What vh_mixtral_decode chains per layer, for a maintainer who binds a single module of HF's MixtralDecoderLayer
// (reached from vita/model/language_model/vita_mixtral.py:158-169) at batch 1.  Scratch is caller-provided; the
// kernels and their arithmetic are the engine's own.
int vh_router_top2(const float* x, long ldx, const uint16_t* Wg, int E, int H, int rows, int* ids, float* wts, float* probs,
                   void* stream) {
    if (!x || !Wg || !ids || !wts) return fail(VH_E_ARG, "vh_router_top2: null pointer");
    return check_launch("vh_router_top2", vhk_router_top2(S(stream), x, ldx, Wg, E, H, rows, ids, wts, probs));
}

// a layer's experts are complete: the three weights, and for the quantised formats their scales
static bool experts_complete(const VhExperts& x) {
    return x.w1 && x.w3 && x.w2 && (x.fmt == VH_EXPERTS_BF16 || (x.s1 && x.s3 && x.s2));
}
static int moe_decode(const char* name, const VhExperts& ex, const float* x, const float* delta, const float* norm_w, float eps,
                      const uint16_t* Wg, int E, int I, int H, float* x_out, float* y, int* route, float* hbuf, void* stream) {
    if (!x || !norm_w || !Wg || !experts_complete(ex) || !y || !route || !hbuf) return fail(VH_E_ARG, "%s: null pointer", name);
    if (H % 64 || I % 64 || H > 14336 || I > 14336) return fail(VH_E_SHAPE, "%s: H, I must be multiples of 64 and <= 14336", name);
    char what[64];
    snprintf(what, sizeof(what), "%s (gate|up)", name);
    int rc = check_launch(what, vhk_dec_gateup(S(stream), x, delta, x_out, norm_w, eps, Wg, E, ex, I, H, route, hbuf, 0));
    if (rc != VH_OK) return rc;
    snprintf(what, sizeof(what), "%s (down)", name);
    return check_launch(what, vhk_dec_down(S(stream), hbuf, route, ex, H, I, y));
}
int vh_moe_decode(const float* x, const float* delta, const float* norm_w, float eps, const uint16_t* Wg, const uint16_t* W1,
                  const uint16_t* W3, const uint16_t* W2, int E, int I, int H, float* x_out, float* y, int* route, float* hbuf,
                  void* stream) {
    const VhExperts ex{VH_EXPERTS_BF16, W1, W3, W2, nullptr, nullptr, nullptr};
    return moe_decode("vh_moe_decode", ex, x, delta, norm_w, eps, Wg, E, I, H, x_out, y, route, hbuf, stream);
}
int vh_moe_decode_i8(const float* x, const float* delta, const float* norm_w, float eps, const uint16_t* Wg, const int8_t* W1,
                     const float* s1, const int8_t* W3, const float* s3, const int8_t* W2, const float* s2, int E, int I, int H,
                     float* x_out, float* y, int* route, float* hbuf, void* stream) {
    const VhExperts ex{VH_EXPERTS_I8, W1, W3, W2, s1, s3, s2};
    return moe_decode("vh_moe_decode_i8", ex, x, delta, norm_w, eps, Wg, E, I, H, x_out, y, route, hbuf, stream);
}
int vh_moe_decode_mxfp4(const float* x, const float* delta, const float* norm_w, float eps, const uint16_t* Wg, const uint8_t* W1,
                        const uint8_t* s1, const uint8_t* W3, const uint8_t* s3, const uint8_t* W2, const uint8_t* s2, int E, int I, int H,
                        float* x_out, float* y, int* route, float* hbuf, void* stream) {
    const VhExperts ex{VH_EXPERTS_MXFP4, W1, W3, W2, s1, s3, s2};
    return moe_decode("vh_moe_decode_mxfp4", ex, x, delta, norm_w, eps, Wg, E, I, H, x_out, y, route, hbuf, stream);
}

int vh_rope_kv_append(const float* qkv, long ldqkv, float* q_out, float* kcache, float* vcache, const float* rope_cos,
                      const float* rope_sin, int Sn, int pos0, int nq, int nkv, int max_ctx, const int* table, void* stream) {
    if (!qkv || !q_out || !kcache || !vcache || !rope_cos || !rope_sin) return fail(VH_E_ARG, "vh_rope_kv_append: null pointer");
    if (Sn < 1 || pos0 < 0 || pos0 + Sn > max_ctx) return fail(VH_E_SHAPE, "vh_rope_kv_append: rows [%d, %d) outside the cache (%d)", pos0, pos0 + Sn, max_ctx);
    return check_launch("vh_rope_kv_append", vhk_rope_kv(S(stream), qkv, ldqkv, q_out, kcache, vcache, rope_cos, rope_sin, Sn, pos0,
                                                         nq, nkv, max_ctx, table, nullptr, 0));
}

int vh_attn_decode(const float* qkv, float* kcache, float* vcache, int pos, const float* rope_cos, const float* rope_sin,
                   int nq, int nkv, int max_ctx, float scale, const int* table, float* part_o, float* part_ml, int* tickets,
                   float* attn_out, void* stream) {
    if (!qkv || !kcache || !vcache || !rope_cos || !rope_sin || !part_o || !part_ml || !tickets || !attn_out)
        return fail(VH_E_ARG, "vh_attn_decode: null pointer");
    if (pos < 0 || pos >= max_ctx) return fail(VH_E_SHAPE, "vh_attn_decode: position %d outside the cache (%d)", pos, max_ctx);
    const int max_splits = (max_ctx + 63) / 64;
    return check_launch("vh_attn_decode", vhk_dec_attn(S(stream), qkv, kcache, vcache, nullptr, rope_cos, rope_sin, part_o, part_ml,
                                                      tickets, attn_out, nq, nkv, max_ctx, max_splits, pos + 1, scale, table));
}

int vh_attn_decode_batch(int n, const float* const* qkv, float* kcache, float* vcache, const int* pos, const float* rope_cos,
                         const float* rope_sin, int nq, int nkv, int max_ctx, float scale, const int* const* table,
                         float* const* part_o, float* const* part_ml, int* const* tickets, float* const* attn_out, void* stream) {
    if (!qkv || !kcache || !vcache || !pos || !rope_cos || !rope_sin || !table || !part_o || !part_ml || !tickets || !attn_out)
        return fail(VH_E_ARG, "vh_attn_decode_batch: null pointer");
    if (n < 1 || n > VH_BMAX) return fail(VH_E_SHAPE, "vh_attn_decode_batch: %d sequences outside [1, %d]", n, VH_BMAX);
    if (nq < 1 || nkv < 1 || max_ctx < 1) return fail(VH_E_SHAPE, "vh_attn_decode_batch: nq, nkv and max_ctx must be positive");
    VhDecBatchAttn at{};
    for (int b = 0; b < n; ++b) {
        if (!qkv[b] || !part_o[b] || !part_ml[b] || !tickets[b] || !attn_out[b])
            return fail(VH_E_ARG, "vh_attn_decode_batch: null pointer (sequence %d)", b);
        if (pos[b] < 0 || pos[b] >= max_ctx)
            return fail(VH_E_SHAPE, "vh_attn_decode_batch: position %d of sequence %d outside the cache (%d)", pos[b], b, max_ctx);
        for (int a = 0; a < b; ++a)      // every sequence has its own scratch and output: the blocks of all of them run side by side
            if (part_o[a] == part_o[b] || part_ml[a] == part_ml[b] || tickets[a] == tickets[b] || attn_out[a] == attn_out[b])
                return fail(VH_E_ARG, "vh_attn_decode_batch: sequences %d and %d share a scratch or output buffer", a, b);
        at.qkv[b] = qkv[b]; at.pos[b] = pos[b]; at.table[b] = table[b];
        at.part_o[b] = part_o[b]; at.part_ml[b] = part_ml[b]; at.cnt[b] = tickets[b]; at.attn_out[b] = attn_out[b];
    }
    const int max_splits = (max_ctx + 63) / 64;
    return check_launch("vh_attn_decode_batch", vhk_decb_attn(S(stream), at, n, kcache, vcache, rope_cos, rope_sin, nq, nkv, max_ctx,
                                                            max_splits, scale));
}

// scratch of vh_attn_rows: the n descriptors (a 256-byte multiple), then the partials
static size_t attn_rows_desc_bytes(int n) { return ((size_t)n * sizeof(VhSeg) + 255) / 256 * 256; }
size_t vh_attn_rows_scratch_bytes(int n, int nq, int max_klen) {
    if (n < 1 || nq < 1 || max_klen < 1) return 0;
    return attn_rows_desc_bytes(n) + vhk_attn_rows_scratch_floats(nq, (max_klen + 63) / 64, n) * sizeof(float);
}
int vh_attn_rows(int n, const float* q, long ldq, const float* kcache, const float* vcache, const int* klens, const int* const* tables,
                 int nq, int nkv, int max_ctx, float scale, void* scratch, size_t scratch_bytes, float* out, uint16_t* out_hi,
                 uint16_t* out_lo, long ldo, void* stream) {
    const char* what = "vh_attn_rows";
    if (!q || !kcache || !vcache || !klens || !tables || !scratch || (!out && !out_hi) || (out_hi && !out_lo) || (out_lo && !out_hi))
        return fail(VH_E_ARG, "%s: null pointer", what);
    if (n < 1 || n > 65535) return fail(VH_E_SHAPE, "%s: %d rows outside [1, 65535]", what, n);
    if (nq < 1 || nkv < 1 || max_ctx < 1 || nq % nkv != 0 || nq / nkv > 4)
        return fail(VH_E_SHAPE, "%s: %d query heads on %d KV heads (1 ... 4 per KV head), pool of %d rows", what, nq, nkv, max_ctx);
    auto al = [](const void* ptr, uintptr_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0; };
    if (!al(q, 16) || !al(kcache, 16) || !al(vcache, 16) || !al(scratch, 16) || !al(out, 8) || !al(out_hi, 4) || !al(out_lo, 4))
        return fail(VH_E_ARG, "%s: misaligned pointer (q, K, V and scratch 16 bytes, out 8, planes 4)", what);
    if (ldq < (long)nq * 128 || (ldq % 4) != 0 || ldo < (long)nq * 128 || (ldo % 2) != 0)
        return fail(VH_E_SHAPE, "%s: row strides %ld / %ld below %d floats or not a multiple of 4 / 2", what, ldq, ldo, nq * 128);
    int kmax = 0;
    for (int i = 0; i < n; ++i) {
        if (klens[i] < 1 || klens[i] > max_ctx) return fail(VH_E_SHAPE, "%s: %d keys of row %d outside [1, %d]", what, klens[i], i, max_ctx);
        if (!tables[i]) return fail(VH_E_ARG, "%s: null page table (row %d)", what, i);
        if (klens[i] > kmax) kmax = klens[i];
    }
    const size_t head = attn_rows_desc_bytes(n);
    if (scratch_bytes < head + vhk_attn_rows_scratch_floats(nq, (kmax + 63) / 64, 1) * sizeof(float))
        return fail(VH_E_SHAPE, "%s: %zu bytes of scratch do not hold the descriptors and one row of %d keys (vh_attn_rows_scratch_bytes)", what,
                    scratch_bytes, kmax);
    std::vector<VhSeg> sg(n);
    for (int i = 0; i < n; ++i) sg[i] = VhSeg{i, 1, klens[i] - 1, 0, tables[i]};
    hipStream_t st = S(stream);
    // the descriptors go up from host memory that ends with this call: the copy is waited for (an operator entry; the engine keeps its
    // descriptors in storage that outlives the pass)
    if (hipMemcpyAsync(scratch, sg.data(), (size_t)n * sizeof(VhSeg), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(VH_E_HIP, "%s: descriptor upload failed", what);
    return check_launch(what, vhk_attn_rows(st, q, ldq, static_cast<const VhSeg*>(scratch), sg.data(), n, kcache, vcache, nq, nkv, max_ctx,
                                            scale, reinterpret_cast<float*>(static_cast<char*>(scratch) + head),
                                            (scratch_bytes - head) / sizeof(float), out, out_hi, out_lo, ldo));
}

int vh_lmhead_argmax(const float* x, const float* delta, const float* norm_w, float eps, const uint16_t* W, int V, int H,
                     float* logits, int* token_out, float* blk_val, int* blk_idx, int nblk, void* stream) {
    if (!x ||!norm_w || !W || !logits || !token_out || !blk_val || !blk_idx) return fail(VH_E_ARG, "vh_lmhead_argmax: null pointer");
    if (nblk < 1 || nblk > 4096 || H % 8) return fail(VH_E_SHAPE, "vh_lmhead_argmax: 1 <= nblk <= 4096, H %% 8 == 0");
    const int grid = nblk < (V + 7) / 8 ? nblk : (V + 7) / 8;
    int rc = check_launch("vh_lmhead_argmax", vhk_dec_lmhead(S(stream), x, delta, norm_w, eps, W, V, H, logits, blk_val, blk_idx, grid,
                                                             nullptr, 1, 0, V));
    if (rc != VH_OK) return rc;
    return check_launch("vh_lmhead_argmax (pick)", vhk_dec_pick(S(stream), blk_val, blk_idx, grid, V, token_out, nullptr));
}

}  // extern "C"

// =========================================================================================
// Mixtral engine
// =========================================================================================
namespace {

// RCCL is resolved at run time (same librccl torch already mapped) so libvita_hip.so has no
// link-time dependency on it and loads on a single-GPU box without RCCL in the path.
struct Id128 { char b[128]; };  // ncclUniqueId is passed BY VALUE (128 bytes)
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id128, int) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;
bool load_rccl() {
    if (g_rccl.lib) return true;
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void* h = nullptr;
    for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_NOLOAD); if (h) break; }
    if (!h) for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) return false;
    g_rccl.GetUniqueId = reinterpret_cast<decltype(g_rccl.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    g_rccl.CommInitRank = reinterpret_cast<decltype(g_rccl.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    g_rccl.AllReduce = reinterpret_cast<decltype(g_rccl.AllReduce)>(dlsym(h, "ncclAllReduce"));
    g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce) return false;
    g_rccl.lib = h;
    return true;
}

inline size_t al(size_t n, size_t a) { return (n + a - 1) & ~(a - 1); }

// Workspace carver.  Buffers of 1 MiB and more start on 2 MiB boundaries (the allocation granule of the device page
// tables); small ones on 256 B.  The ORDER in vh_mixtral::carve is part of the performance contract: everything the
// prefill kernels stream sits in front of the KV cache, so its placement does not move with max_new / max_ctx.  (r03 measurement,
// profiles/r03_layout_*: prefill time does NOT depend on the placement — 52.5 ms under three step settings and five pads
// on one box, 40.0 ms under two on another; the r02 "39.7 vs 52.6 ms" was the box, not the layout.)
struct Carver {
    char* base; size_t off;
    template <typename T> T* take(size_t count) {
        const size_t bytes = count * sizeof(T);
        off = al(off, bytes >= (1u << 20) ? (size_t(2) << 20) : size_t(256));
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += bytes;
        return p;
    }
};

}  // namespace

struct vh_mixtral {
    vh_mixtral_cfg c;
    std::vector<vh_mixtral_layer> L;
    std::vector<VhExperts> X;   // the experts of every layer in the engine's format (vh_kernels.h): L[l].w1 / w3 / w2 are read through it only
    const uint16_t* embed; const float* final_norm; const uint16_t* lm_head;
    const float* rope_cos; const float* rope_sin;
    int nq, nkv, hd, H, I, E, V, nqkv, max_splits, lm_grid;
    int v0 = 0, Vn = 0;         // this rank's rows of the LM head ([v0, v0 + Vn); the whole table when unsharded)
    float* cand = nullptr;      // [tp_world][2] (value, index) candidates of the vocab-sharded head
    // state (xa .. delta_moe, counters, out_tokens: where carve() puts the single-sequence engine's; read through units[0])
    float *kcache, *vcache;  // [layer][nkv][max_ctx][hd]
    float *xa, *xb, *delta_attn, *delta_moe, *qkv, *part_o, *part_ml, *attn_out, *hbuf, *logits, *blk_val;
    int *blk_idx, *route, *counters, *out_tokens, *attn_cnt;
    // prefill scratch
    float *px, *pxn, *pqkv, *pq, *pattn, *py, *ptmp, *pwts;
    uint16_t *pxn_hi, *pxn_lo, *ph_hi, *ph_lo;   // bf16 hi/lo planes feeding the pre-split MoE GEMMs
    unsigned char* kv_img = nullptr; int img_tiles = 0;   // K / V tile images (VhAttnArgs::kv_img) of a one-shot prefill
    int *pids, *pgoff, *pstok, *psslot, *pnslab;
    // ---- concurrent sequences over a paged KV cache (vLLM's block tables).  The KV pool above is cut into
    // 64-token pages (= one decode-attention tile); a sequence owns a page table, a residual-stream state, its counters
    // and its generated ids.  All of it is reached through ONE record per state owner (Unit): units[0] is the single-sequence
    // engine, units[1 + s] sequence slot s.  Prefill, a decode step and the head take the unit they work on, so they are the
    // same code for both; the batched iteration and the batched prefill take a list of units.
    // logit rules of one request (vh_logit_rules): penalties read the request's token table, K >= 0 runs k_dec_logprobs after the select
    struct Rules {
        float r = 1.f, f = 0.f, p = 0.f; int K = -1;
        bool pen() const { return r != 1.f || f != 0.f || p != 0.f; }
    };
    struct Unit {
        // device buffers, fixed once init_units() has run
        float *xa = nullptr, *xb = nullptr, *da = nullptr, *dm = nullptr;   // residual stream in / out, attention delta, MoE delta ([H] each)
        int *counters = nullptr;           // {pos, n_generated, attn_done (monotonic), device error flag}
        int *tokens = nullptr;             // [lp_rows()] generated ids
        int *table = nullptr;              // [max_splits] page table; null = contiguous rows (unit 0)
        unsigned* seen = nullptr;          // [V] token table of the penalties (cfg.penalty_tables, else null)
        float *lp_tok = nullptr, *lp_top = nullptr; int* lp_top_id = nullptr;   // [lp_rows()] / [lp_rows()][max_logprobs] (cfg.max_logprobs, else null)
        // host mirrors
        int host_pos = 0;                  // mirror of counters[0] (sizes the split-KV grid without a device read)
        int poisoned = 0;                  // a step was enqueued in part: unit 0 needs a prefill / reset, a slot is lost until freed
        bool seen_dirty = false;           // the token table holds a history (a setter call without penalties clears it)
        VhSampleParams samp{};             // vh_mixtral_[seq_]set_sampling (T = 0: greedy)
        Rules rules{};                     // vh_mixtral_[seq_]set_logit_rules (off)
        VhPenalty pen() const { return rules.pen() ? VhPenalty{seen, rules.r, rules.f, rules.p, 0} : VhPenalty{}; }
        // what reset / seq_alloc / seq_free leave: position 0, greedy, no logit rules
        void fresh() { host_pos = 0; poisoned = 0; samp = VhSampleParams{}; rules = Rules{}; }
    };
    std::vector<Unit> units;               // [1 + max_seqs]
    Unit& slot(int s) { return units[1 + s]; }
    const Unit& slot(int s) const { return units[1 + s]; }
    struct Seq {                           // paging state of slot s (the rest of the slot is units[1 + s])
        bool live = false;
        int npages = 0;
        std::vector<int> pages;            // host mirror of the device table (sized once: uploads read from it)
    };
    std::vector<Seq> seqs;
    std::vector<int> free_pages;
    // Reference counts of the pages (host memory): a sequence that has the page in its table counts 1, every hold
    // (vh_mixtral_seq_hold_prefix) counts 1; a page is on the free list exactly when its count is 0.
    // INVARIANT: the engine never writes a row of a page whose count is above 1.  It holds because (1) vh_mixtral_seq_adopt starts a
    // sequence on a page boundary, behind the pages it shares; (2) a hold covers only full pages below its owner's position; (3) a
    // sequence writes K/V only at or above its own position (prefill appends at host_pos, a decode step writes row host_pos).
    std::vector<int> page_refs;
    int take_page() { const int pg = free_pages.back(); free_pages.pop_back(); page_refs[pg] = 1; return pg; }
    void unref_page(int pg) { if (--page_refs[pg] == 0) free_pages.push_back(pg); }
    bool pages_in_use() const { return (int)free_pages.size() < n_pages(); }
    std::vector<int> batch_ids_host;   // slot list last uploaded to seq_batch (storage reserved once)
    std::vector<VhSeg> segs_host;      // segment descriptors of the current batched prefill pass (storage reserved once: uploads read from it)
    VhSeg* seq_segs = nullptr;         // [max_seqs] the same on the device
    float* seq_x = nullptr;            // [max_seqs][4][H]: xa, xb, delta_attn, delta_moe
    int *seq_counters = nullptr, *seq_tokens = nullptr, *seq_table = nullptr, *seq_batch = nullptr;
    // scratch "lanes" of the per-step buffers for batched decode iterations: lane 0 = the single-sequence ones, lanes 1..VH_BMAX-1
    // exist only with sequence slots
    float *l_qkv[VH_BMAX] = {}, *l_part_o[VH_BMAX] = {}, *l_part_ml[VH_BMAX] = {}, *l_attn_out[VH_BMAX] = {}, *l_hbuf[VH_BMAX] = {},
          *l_blk_val[VH_BMAX] = {}, *l_cand[VH_BMAX] = {};
    int *l_attn_cnt[VH_BMAX] = {}, *l_route[VH_BMAX] = {}, *l_blk_idx[VH_BMAX] = {};
    // state of the logit rules, one row per unit
    unsigned* seen_tab = nullptr;      // [1 + max_seqs][V] token tables (cfg.penalty_tables)
    float *lp_tok = nullptr, *lp_top = nullptr; int* lp_top_id = nullptr;   // [1 + max_seqs][max_new] / [..][max_new][max_logprobs]
    int device = -1;                   // the device the workspace lives on (the setters synchronise THAT device)
    int lp_rows() const { return c.max_new > 0 ? c.max_new : 1; }   // rows of a unit's token / logprob buffers
    void logprob_slot(VhDecLogprobJob& j, const Unit& u, const float* row) const {
        const int q = j.n++;
        j.logits[q] = row; j.ngen[q] = u.counters + 1; j.tokens[q] = u.tokens; j.K[q] = u.rules.K;
        j.lp_tok[q] = u.lp_tok; j.lp_top_id[q] = u.lp_top_id; j.lp_top[q] = u.lp_top;
    }
    float* samp_rows = nullptr;        // [VH_BMAX][V] logits rows of the batched head for sequences with a top-k / top-p filter
    int n_pages() const { return c.max_ctx / 64; }
    int live_seqs() const { int n = 0; for (const Seq& q : seqs) n += q.live; return n; }
    // pages covering positions [0, n_tokens) of sequence s; new table entries are uploaded on st.  -1: pool exhausted.
    int ensure_pages(int s, int n_tokens, hipStream_t st) {
        Seq& q = seqs[s];
        const int need = (n_tokens + 63) / 64, had = q.npages;
        if (need <= had) return 0;
        if (need > max_splits || (int)free_pages.size() < need - had) return -1;
        for (int j = had; j < need; ++j) q.pages[j] = take_page();
        q.npages = need;
        if (hipMemcpyAsync(slot(s).table + had, q.pages.data() + had, (size_t)(need - had) * sizeof(int),
                           hipMemcpyHostToDevice, st) != hipSuccess) return -2;
        return 0;
    }
    void release(int s) {
        Seq& q = seqs[s];
        for (int j = q.npages - 1; j >= 0; --j) unref_page(q.pages[j]);
        q.npages = 0; q.live = false;
        slot(s).fresh();
    }
    void init_seqs() {
        seqs.assign(c.max_seqs > 0 ? c.max_seqs : 0, Seq{});
        for (Seq& q : seqs) q.pages.assign(max_splits, 0);
        free_pages.clear();
        for (int pg = n_pages() - 1; pg >= 0; --pg) free_pages.push_back(pg);   // page 0 is handed out first
        page_refs.assign(n_pages() > 0 ? n_pages() : 0, 0);
        batch_ids_host.clear();
        batch_ids_host.reserve(seqs.size() + 1);
        segs_host.clear();
        segs_host.reserve(seqs.size() + 1);
    }
    // the records, from the buffers carve() handed out: the one place that knows how the slots lie in seq_x .. seq_table and the
    // rules buffers
    void init_units() {
        const size_t rows = (size_t)lp_rows(), top = rows * (size_t)c.max_logprobs;
        units.assign(1 + seqs.size(), Unit{});
        for (size_t i = 0; i < units.size(); ++i) {
            Unit& u = units[i];
            if (i == 0) {
                u.xa = xa; u.xb = xb; u.da = delta_attn; u.dm = delta_moe;
                u.counters = counters; u.tokens = out_tokens;
            } else {
                const size_t s = i - 1;
                float* x = seq_x + s * 4 * H;
                u.xa = x; u.xb = x + H; u.da = x + 2 * H; u.dm = x + 3 * H;
                u.counters = seq_counters + 4 * s;
                u.tokens = seq_tokens + s * rows;
                u.table = seq_table + s * max_splits;
            }
            if (seen_tab) u.seen = seen_tab + i * V;
            if (lp_tok) { u.lp_tok = lp_tok + i * rows; u.lp_top_id = lp_top_id + i * top; u.lp_top = lp_top + i * top; }
        }
    }
    int rccl_gen = 0;           // bumped by vh_mixtral_cancel_rccl: a pending vh_mixtral_init_rccl then discards its communicator
    int* route_dbg = nullptr;   // optional: per-layer top-2 expert ids of the next prefill, [layer][token][2]
    // tensor parallel
    vh_allreduce_fn ar_fn; void* ar_user; void* rccl_comm;
    // optional live timing of the dominant decode kernel (gate/up GEMV), sampled every prof_stride layers
    int prof_stride = 0;
    std::vector<hipEvent_t> prof_ev;  // start/stop pairs
    size_t prof_used = 0;

    size_t carve(void* ws) {
        Carver cv{reinterpret_cast<char*>(ws), 0};
        const size_t Sm = (size_t)c.max_prefill;
        // ---- prefill scratch first: fixed offsets for a given (max_prefill, geometry) --------------------------------
        pxn_hi = cv.take<uint16_t>(Sm * H); pxn_lo = cv.take<uint16_t>(Sm * H);
        // ph planes: the MoE's h rows (2 S x I) and, before them in each layer, the attention output rows (S x nq hd) that feed the
        // O projection — whichever is wider (nq hd > 2 I at small intermediate widths)
        const size_t ph_cols = 2 * (size_t)I > (size_t)nq * hd ? 2 * (size_t)I : (size_t)nq * hd;
        ph_hi = cv.take<uint16_t>(Sm * ph_cols); ph_lo = cv.take<uint16_t>(Sm * ph_cols);
        px = cv.take<float>(Sm * H); pxn = cv.take<float>(Sm * H);
        pqkv = cv.take<float>(Sm * nqkv);
        pq = cv.take<float>(Sm * nq * hd); pattn = cv.take<float>(Sm * nq * hd);
        py = cv.take<float>(4 * (size_t)down_slab(H));   // up to 4 K-split slabs of the MoE down projection / 8 of the projections
        ptmp = cv.take<float>(Sm * H);
        pwts = cv.take<float>(2 * Sm);
        pids = cv.take<int>(2 * Sm); pgoff = cv.take<int>(E + 1);
        pstok = cv.take<int>(2 * Sm); psslot = cv.take<int>(2 * Sm);
        pnslab = cv.take<int>(4);
        // K / V tile images of a one-shot prefill for the flash attention kernel (64 KB per KV head and 64-row tile; only when the
        // head grouping is the 4 : 1 that kernel serves)
        img_tiles = (nq == 4 * nkv && hd == 128) ? (c.max_prefill + 63) / 64 : 0;
        kv_img = img_tiles ? cv.take<unsigned char>((size_t)nkv * img_tiles * 65536) : nullptr;
        // ---- decode state ------------------------------------------------------------------------------------------
        xa = cv.take<float>(H); xb = cv.take<float>(H);
        delta_attn = cv.take<float>(H); delta_moe = cv.take<float>(H);
        qkv = cv.take<float>(nqkv);
        attn_out = cv.take<float>((size_t)nq * hd);
        attn_cnt = cv.take<int>(nkv);  // arrival tickets; zero at creation, reset by each last arriver
        hbuf = cv.take<float>((size_t)2 * I);
        blk_val = cv.take<float>(3 * (size_t)lm_grid);   // greedy: one value per block; sampled: 3-float keys (vh_sample.h vhs_key3)
        blk_idx = cv.take<int>(lm_grid);
        cand = cv.take<float>(4 * (c.tp_world > 0 ? c.tp_world : 1));
        route = cv.take<int>(4);
        counters = cv.take<int>(4);  // {pos, n_generated, attn_done (monotonic), device error flag}
        g_qkv = cv.take<unsigned long long>(nqkv);
        g_attn = cv.take<unsigned long long>(vh_gran_gemv_len(nq * hd));
        // ---- everything whose size follows max_ctx / max_new / logit_rows: behind the fixed part ---------------------------
        out_tokens = cv.take<int>(lp_rows());
        part_o = cv.take<float>((size_t)nq * max_splits * hd);
        part_ml = cv.take<float>((size_t)nq * max_splits * 2);
        logits = cv.take<float>((size_t)hist_rows() * V);
        l_qkv[0] = qkv; l_part_o[0] = part_o; l_part_ml[0] = part_ml; l_attn_out[0] = attn_out; l_attn_cnt[0] = attn_cnt;
        l_hbuf[0] = hbuf; l_route[0] = route; l_blk_val[0] = blk_val; l_blk_idx[0] = blk_idx; l_cand[0] = cand;
        if (c.max_seqs > 0) {
            const size_t n = (size_t)c.max_seqs;
            seq_x = cv.take<float>(n * 4 * H);
            seq_counters = cv.take<int>(n * 4);
            seq_tokens = cv.take<int>(n * lp_rows());
            seq_table = cv.take<int>(n * max_splits);
            seq_batch = cv.take<int>(n);
            seq_segs = cv.take<VhSeg>(n);   // 24 bytes per slot: the segments of a batched prefill pass
            for (int b = 1; b < VH_BMAX; ++b) {
                l_qkv[b] = cv.take<float>(nqkv);
                l_part_o[b] = cv.take<float>((size_t)nq * max_splits * hd);
                l_part_ml[b] = cv.take<float>((size_t)nq * max_splits * 2);
                l_attn_out[b] = cv.take<float>((size_t)nq * hd);
                l_attn_cnt[b] = cv.take<int>(nkv);
                l_hbuf[b] = cv.take<float>((size_t)2 * I);
                l_route[b] = cv.take<int>(4);
                l_blk_val[b] = cv.take<float>(3 * (size_t)lm_grid);
                l_blk_idx[b] = cv.take<int>(lm_grid);
                l_cand[b] = cv.take<float>(4 * (c.tp_world > 0 ? c.tp_world : 1));
            }
            samp_rows = cv.take<float>((size_t)VH_BMAX * V);
        }
        kcache = cv.take<float>((size_t)c.n_layers * nkv * c.max_ctx * hd);
        vcache = cv.take<float>((size_t)c.n_layers * nkv * c.max_ctx * hd);
        // ---- logit rules (behind everything else: an engine without them is laid out as before) -----------------------------
        const size_t units = 1 + (size_t)(c.max_seqs > 0 ? c.max_seqs : 0);
        if (c.penalty_tables) seen_tab = cv.take<unsigned>(units * V);
        if (c.max_logprobs > 0) {
            lp_tok = cv.take<float>(units * lp_rows());
            lp_top_id = cv.take<int>(units * lp_rows() * c.max_logprobs);
            lp_top = cv.take<float>(units * lp_rows() * c.max_logprobs);
        }
        return al(cv.off, 256);
    }
    // py layout: a K-split slab of a projection output (QKV, O) `ncols` wide holds max_prefill rows, one of the MoE down
    // projection 2 max_prefill (a row per routed token slot); the overlapped tensor-parallel steps keep the slabs of column
    // half h of the O / down projection from py_half(h) on (py_half(0) is py itself)
    long proj_slab(long ncols) const { return (long)c.max_prefill * ncols; }
    long down_slab(long ncols) const { return 2L * c.max_prefill * ncols; }
    float* py_half(int h) const { return py + (size_t)h * 8 * c.max_prefill * (H / 2); }
    int hist_rows() const { return c.logit_rows > 1 ? c.logit_rows : 1; }
    int cand_world() const { return c.tp_world > 1 ? c.tp_world : 1; }   // slots of the vocab-sharded head's candidate vector (loop-back: this rank's only)
    // The head's candidates are exchanged: the LM head is a vocab shard of a tensor-parallel rank.  The single-sequence form also
    // counts a loop-back communicator (one rank playing them all); the batched callers never did.
    bool head_sharded(bool loopback_counts) const {
        return c.vocab_n > 0 && (c.tp_world > 1 || (loopback_counts && comm && vh_comm_is_loopback(comm)));
    }
    void derive() {
        nq = c.n_q_heads; nkv = c.n_kv_heads; hd = c.head_dim; H = c.hidden; I = c.inter; E = c.n_experts;
        V = c.vocab; nqkv = (nq + 2 * nkv) * hd;
        max_splits = (c.max_ctx + 63) / 64;
        v0 = c.vocab_n > 0 ? c.vocab_lo : 0;
        Vn = c.vocab_n > 0 ? c.vocab_n : V;
        lm_grid = (Vn + 7) / 8;
        if (lm_grid > 1024) lm_grid = 1024;
        if (lm_grid < c.tp_world) lm_grid = c.tp_world;   // blk_val / blk_idx also hold the gathered candidates
    }
    // ---- fused attention-block launch (k_dec_ablk): q|k|v and the attention output travel between its work items as
    // tagged granules; a tag is used once per (step, layer, vector)
    unsigned long long *g_qkv = nullptr, *g_attn = nullptr;   // granule vectors (VhGranVec)
    unsigned gran_epoch = 0;                         // last granule tag handed out (0 = never written)
    int schedule_state = -1;                         // attention block of the last decode call: -1 none yet, 0 three launches, 1 one fused launch
    unsigned next_tag() { if (++gran_epoch == 0) ++gran_epoch; return gran_epoch; }
    vh_comm_t* comm = nullptr;   // the library's IPC all-reduce (not owned)
    hipStream_t cs = nullptr;    // communication stream of the overlapped tensor-parallel prefill
    hipEvent_t ev_c[2] = {nullptr, nullptr}, ev_r[2] = {nullptr, nullptr};   // half computed / half reduced
    // the collective can run on another stream than the compute stream (native RCCL, IPC) — the Python callback cannot
    bool stream_capable() const { return comm != nullptr || rccl_comm != nullptr; }
    int ensure_comm_stream() {
        if (cs) return 0;
        if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) return -1;
        for (int i = 0; i < 2; ++i)
            if (hipEventCreateWithFlags(&ev_c[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ev_r[i], hipEventDisableTiming) != hipSuccess) return -1;
        return 0;
    }
    // exchanges run: a tensor-parallel rank, a test that forces the hook, or a loop-back communicator (one rank playing them all)
    bool exchanges() const { return c.tp_world > 1 || vh_tuning()->force_allreduce || (comm && vh_comm_is_loopback(comm)); }
    int allreduce(float* buf, long count, hipStream_t st) {
        if (!exchanges()) return 0;
        if (comm && (size_t)count <= vh_comm_capacity(comm)) return vh_comm_allreduce(comm, buf, count, st) == VH_OK ? 0 : -1;
        if (!ar_fn) return -1;
        return ar_fn(ar_user, buf, count, st);
    }
};

namespace {
int cfg_ok(const vh_mixtral_cfg* c) {
    if (!c) return fail(VH_E_ARG, "null cfg");
    if (c->head_dim != 128) return fail(VH_E_SHAPE, "head_dim must be 128 (got %d)", c->head_dim);
    if (c->top_k != 2) return fail(VH_E_SHAPE, "top_k must be 2");
    if (c->n_experts < 2 || c->n_experts > 8) return fail(VH_E_SHAPE, "n_experts must be in [2,8]");
    if (c->hidden % 64 || c->inter % 64) return fail(VH_E_SHAPE, "hidden and inter must be multiples of 64");
    if (c->hidden > 14336 || c->inter > 14336 || c->n_q_heads * c->head_dim > 14336)
        return fail(VH_E_SHAPE, "dimension above the GEMV register budget (14336)");
    if (c->n_q_heads % c->n_kv_heads || c->n_q_heads / c->n_kv_heads > 4)
        return fail(VH_E_SHAPE, "GQA group must divide and be <= 4");
    if (c->max_ctx < 1 || c->max_prefill < 1 || c->n_layers < 1) return fail(VH_E_SHAPE, "bad sizes");
    if (c->vocab_n < 0 || c->vocab_lo < 0 || (c->vocab_n > 0 && c->vocab_lo + c->vocab_n > c->vocab))
        return fail(VH_E_SHAPE, "vocab shard outside the table");
    if (c->vocab_n > 0 && c->vocab >= (1 << 24)) return fail(VH_E_SHAPE, "vocab-sharded head needs vocab < 2^24");
    if (c->max_seqs < 0 || c->max_seqs > 4096) return fail(VH_E_SHAPE, "max_seqs outside [0,4096]");
    if (c->max_seqs > 0 && (c->max_ctx % 64) != 0) return fail(VH_E_SHAPE, "paged KV cache: max_ctx must be a multiple of the 64-token page");
    if (c->max_logprobs < 0 || c->max_logprobs > 20) return fail(VH_E_SHAPE, "max_logprobs outside [0,20]");
    return VH_OK;
}
int rccl_allreduce_cb(void* user, float* buf, long count, void* stream) {
    vh_mixtral* m = reinterpret_cast<vh_mixtral*>(user);
    const int rc = g_rccl.AllReduce(buf, buf, (size_t)count, /*ncclFloat32*/ 7, /*ncclSum*/ 0, m->rccl_comm,
                                    reinterpret_cast<hipStream_t>(stream));
    return rc == 0 ? 0 : -1;
}
// The three creates: `record(l)` is layer l's experts as the entry was given them (bf16: the pointers of layers[l]; quantised: its
// experts[l], and then layers[l] must not name bf16 experts as well); `experts` is the entry's per-layer array, refused when null
int experts_ok(const char* name, int l, const vh_mixtral_layer& w, const VhExperts& x) {
    const bool quantised = x.fmt != VH_EXPERTS_BF16;
    if (quantised && (w.w1 || w.w3 || w.w2))
        return fail(VH_E_ARG, "%s: layers[%d].w1 / w3 / w2 must be null (the experts are quantised: experts[%d])", name, l, l);
    if (!experts_complete(x))
        return fail(VH_E_ARG, "%s: null expert weight or scale pointer in %s[%d]", name, quantised ? "experts" : "layers", l);
    return VH_OK;
}
template <class Record>
vh_mixtral_t* create_engine(const char* name, const vh_mixtral_cfg* cfg, const vh_mixtral_layer* layers, const void* experts,
                            Record&& record, const uint16_t* embed, const float* final_norm, const uint16_t* lm_head,
                            const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes) {
    if (cfg_ok(cfg) != VH_OK) return nullptr;
    if (!layers || !experts || !embed || !final_norm || !lm_head || !rope_cos || !rope_sin || !workspace) {
        fail(VH_E_ARG, "%s: null pointer (layers / experts / tables / workspace)", name);
        return nullptr;
    }
    std::vector<VhExperts> X(cfg->n_layers);
    for (int l = 0; l < cfg->n_layers; ++l) {
        X[l] = record(l);
        if (experts_ok(name, l, layers[l], X[l]) != VH_OK) return nullptr;
    }
    vh_mixtral* m = new vh_mixtral{};
    m->c = *cfg;
    m->derive();
    m->L.assign(layers, layers + cfg->n_layers);
    m->X = std::move(X);
    m->embed = embed; m->final_norm = final_norm; m->lm_head = lm_head;
    m->rope_cos = rope_cos; m->rope_sin = rope_sin;
    m->ar_fn = nullptr; m->ar_user = nullptr; m->rccl_comm = nullptr;
    const size_t need = m->carve(workspace);
    if (need > workspace_bytes) {
        fail(VH_E_ARG, "%s: workspace too small (%zu < %zu)", name, workspace_bytes, need);
        delete m;
        return nullptr;
    }
    m->init_seqs();
    m->init_units();
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, workspace) == hipSuccess) m->device = at.device;
    else (void)hipGetLastError();      // a host pointer (argument tests without a GPU): the current device is used
    return m;
}
}  // namespace

extern "C" {

size_t vh_mixtral_workspace_bytes(const vh_mixtral_cfg* cfg) {
    if (cfg_ok(cfg) != VH_OK) return 0;
    vh_mixtral tmp{};
    tmp.c = *cfg;
    tmp.derive();
    return tmp.carve(nullptr);
}

vh_mixtral_t* vh_mixtral_create(const vh_mixtral_cfg* cfg, const vh_mixtral_layer* layers, const uint16_t* embed,
                                const float* final_norm, const uint16_t* lm_head, const float* rope_cos,
                                const float* rope_sin, void* workspace, size_t workspace_bytes) {
    auto record = [&](int l) { return VhExperts{VH_EXPERTS_BF16, layers[l].w1, layers[l].w3, layers[l].w2, nullptr, nullptr, nullptr}; };
    return create_engine("vh_mixtral_create", cfg, layers, layers, record, embed, final_norm, lm_head, rope_cos, rope_sin, workspace,
                         workspace_bytes);
}

vh_mixtral_t* vh_mixtral_create_i8(const vh_mixtral_cfg* cfg, const vh_mixtral_layer* layers, const vh_mixtral_experts_i8* experts,
                                   const uint16_t* embed, const float* final_norm, const uint16_t* lm_head, const float* rope_cos,
                                   const float* rope_sin, void* workspace, size_t workspace_bytes) {
    auto record = [&](int l) { const auto& q = experts[l]; return VhExperts{VH_EXPERTS_I8, q.w1, q.w3, q.w2, q.s1, q.s3, q.s2}; };
    return create_engine("vh_mixtral_create_i8", cfg, layers, experts, record, embed, final_norm, lm_head, rope_cos, rope_sin, workspace,
                         workspace_bytes);
}

vh_mixtral_t* vh_mixtral_create_mxfp4(const vh_mixtral_cfg* cfg, const vh_mixtral_layer* layers,
                                      const vh_mixtral_experts_mxfp4* experts, const uint16_t* embed, const float* final_norm,
                                      const uint16_t* lm_head, const float* rope_cos, const float* rope_sin, void* workspace,
                                      size_t workspace_bytes) {
    auto record = [&](int l) { const auto& q = experts[l]; return VhExperts{VH_EXPERTS_MXFP4, q.w1, q.w3, q.w2, q.s1, q.s3, q.s2}; };
    return create_engine("vh_mixtral_create_mxfp4", cfg, layers, experts, record, embed, final_norm, lm_head, rope_cos, rope_sin, workspace,
                         workspace_bytes);
}

void vh_mixtral_destroy(vh_mixtral_t* m) {
    if (!m) return;
    for (hipEvent_t e : m->prof_ev) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) { if (m->ev_c[i]) (void)hipEventDestroy(m->ev_c[i]); if (m->ev_r[i]) (void)hipEventDestroy(m->ev_r[i]); }
    if (m->cs) (void)hipStreamDestroy(m->cs);
    if (m->rccl_comm && g_rccl.CommDestroy) g_rccl.CommDestroy(m->rccl_comm);
    delete m;
}

int vh_mixtral_set_allreduce(vh_mixtral_t* m, vh_allreduce_fn fn, void* user) {
    if (!m) return fail(VH_E_ARG, "null engine");
    m->ar_fn = fn; m->ar_user = user;
    return VH_OK;
}

int vh_rccl_unique_id(void* out) {
    if (!load_rccl()) return fail(VH_E_COMM, "librccl.so not loadable: %s", dlerror());
    const int rc = g_rccl.GetUniqueId(out);
    return rc == 0 ? VH_OK : fail(VH_E_COMM, "ncclGetUniqueId failed (%d)", rc);
}

int vh_mixtral_init_rccl(vh_mixtral_t* m, const void* uid) {
    if (!m || !uid) return fail(VH_E_ARG, "null argument");
    if (!load_rccl()) return fail(VH_E_COMM, "librccl.so not loadable");
    Id128 id;
    memcpy(id.b, uid, 128);
    void* comm = nullptr;
    const int gen = __atomic_load_n(&m->rccl_gen, __ATOMIC_ACQUIRE);
    const int rc = g_rccl.CommInitRank(&comm, m->c.tp_world, id, m->c.tp_rank);
    if (rc != 0) return fail(VH_E_COMM, "ncclCommInitRank failed (%d)", rc);
    // a caller that gave up on this attempt (vh_mixtral_cancel_rccl: bring-up time-out, the ranks agreed on another
    // collective) must not find the communicator installed later, in the middle of a run
    if (__atomic_load_n(&m->rccl_gen, __ATOMIC_ACQUIRE) != gen) {
        if (g_rccl.CommDestroy) g_rccl.CommDestroy(comm);
        return fail(VH_E_COMM, "RCCL bring-up was cancelled");
    }
    m->rccl_comm = comm;
    m->ar_fn = rccl_allreduce_cb; m->ar_user = m;
    return VH_OK;
}

int vh_mixtral_use_comm(vh_mixtral_t* m, vh_comm_t* c) {
    if (!m) return fail(VH_E_ARG, "null engine");
    m->comm = c;
    return VH_OK;
}

int vh_mixtral_cancel_rccl(vh_mixtral_t* m) {
    if (!m) return fail(VH_E_ARG, "null engine");
    __atomic_add_fetch(&m->rccl_gen, 1, __ATOMIC_ACQ_REL);
    return VH_OK;
}

int vh_mixtral_route_debug(vh_mixtral_t* m, int* ids_out) {
    if (!m) return fail(VH_E_ARG, "null engine");
    m->route_dbg = ids_out;   // device int[n_layers][S][2] filled by the following prefill calls; null = off
    return VH_OK;
}

int vh_mixtral_profile(vh_mixtral_t* m, int stride, int max_samples) {
    if (!m) return fail(VH_E_ARG, "null engine");
    m->prof_stride = stride;
    m->prof_used = 0;
    while ((int)m->prof_ev.size() < 2 * max_samples) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return fail(VH_E_HIP, "hipEventCreate failed");
        m->prof_ev.push_back(e);
    }
    return VH_OK;
}

int vh_mixtral_profile_read(vh_mixtral_t* m, double* total_ms, int* count) {
    if (!m || !total_ms || !count) return fail(VH_E_ARG, "null argument");
    double tot = 0.0;
    int n = 0;
    for (size_t i = 0; i + 1 < m->prof_used; i += 2) {
        float ms = 0.f;
        if (hipEventSynchronize(m->prof_ev[i + 1]) != hipSuccess) return fail(VH_E_HIP, "event sync failed");
        if (hipEventElapsedTime(&ms, m->prof_ev[i], m->prof_ev[i + 1]) != hipSuccess)
            return fail(VH_E_HIP, "hipEventElapsedTime failed");
        tot += ms; ++n;
    }
    *total_ms = tot; *count = n;
    m->prof_used = 0;
    return VH_OK;
}

const int* vh_mixtral_tokens(const vh_mixtral_t* m) { return m ? m->units[0].tokens : nullptr; }
const int* vh_mixtral_counters(const vh_mixtral_t* m) { return m ? m->units[0].counters : nullptr; }
const float* vh_mixtral_logits(const vh_mixtral_t* m) { return m ? m->logits : nullptr; }

int vh_mixtral_reset(vh_mixtral_t* m, void* stream) {
    if (!m) return fail(VH_E_ARG, "null engine");
    if (hipMemsetAsync(m->units[0].counters, 0, 4 * sizeof(int), S(stream)) != hipSuccess)
        return fail(VH_E_HIP, "reset memset failed");
    m->units[0].fresh();                         // greedy again, no logit rules (released sequences too)
    for (int s = 0; s < (int)m->seqs.size(); ++s)
        if (m->seqs[s].live) m->release(s);      // the pool is one: a reset returns every page
    if (m->pages_in_use())                       // ... the held ones too (vh_mixtral_seq_hold_prefix): highest id first, so the lowest is
        for (int pg = m->n_pages() - 1; pg >= 0; --pg)   // handed out first among them
            if (m->page_refs[pg] > 0) { m->page_refs[pg] = 0; m->free_pages.push_back(pg); }
    return VH_OK;
}

// a top-k / top-p filter is in force (the temperature-only draw folds into the LM head's per-block argmax)
static bool sampling_filters(const VhSampleParams& p, int V) { return p.T > 0.0 && ((p.top_k > 0 && p.top_k < V) || p.top_p < 1.0); }
// vh_sampling -> kernel parameters (T = 0 or null: greedy)
static int sampling_params(const vh_sampling* s, VhSampleParams* out, const char* what) {
    *out = VhSampleParams{};
    if (!s) return VH_OK;
    if (!std::isfinite(s->temperature) || s->temperature < 0.f) return fail(VH_E_ARG, "%s: temperature must be finite and >= 0 (got %g)", what, (double)s->temperature);
    if (s->top_k < 0) return fail(VH_E_ARG, "%s: top_k must be >= 0 (got %d)", what, s->top_k);
    if (!(s->top_p > 0.f && s->top_p <= 1.f)) return fail(VH_E_ARG, "%s: top_p must be in (0, 1] (got %g)", what, (double)s->top_p);
    if (s->temperature == 0.f) return VH_OK;
    out->T = s->temperature; out->top_p = s->top_p; out->top_k = s->top_k;
    out->seed = s->seed; out->draw0 = s->draw0;
    return VH_OK;
}
static int engine_sampling(const vh_mixtral* m, const vh_sampling* s, VhSampleParams* out, const char* what) {
    const int rc = sampling_params(s, out, what);
    if (rc != VH_OK) return rc;
    // a vocab-sharded head sees its slice only: the temperature-only draw travels through the candidate exchange, a filter cannot
    if (m->c.vocab_n > 0 && m->c.vocab_n < m->V && sampling_filters(*out, m->V))
        return fail(VH_E_ARG, "%s: top-k / top-p need an unsharded LM head (vocab_n = %d of %d)", what, m->c.vocab_n, m->V);
    if (m->c.vocab_n > 0 && m->c.tp_world > 64 && out->T > 0.0)
        return fail(VH_E_ARG, "%s: sampling under a vocab-sharded head takes at most 64 ranks (tp_world %d)", what, m->c.tp_world);
    return VH_OK;
}

int vh_mixtral_set_sampling(vh_mixtral_t* m, const vh_sampling* s) {
    if (!m) return fail(VH_E_ARG, "null engine");
    VhSampleParams p;
    const int rc = engine_sampling(m, s, &p, "vh_mixtral_set_sampling");
    if (rc != VH_OK) return rc;
    m->units[0].samp = p;
    return VH_OK;
}

int vh_sample_rows(const float* logits, long ld, int rows, int V, const vh_sampling* s, int* tokens_out, void* stream) {
    if (!logits || !tokens_out) return fail(VH_E_ARG, "vh_sample_rows: null pointer");
    if (rows < 1 || V < 1 || ld < 0) return fail(VH_E_SHAPE, "vh_sample_rows: rows %d, V %d, ld %ld", rows, V, ld);
    VhSampleParams p;
    const int rc = sampling_params(s, &p, "vh_sample_rows");
    if (rc != VH_OK) return rc;
    return check_launch("vh_sample_rows", vhk_sample_rows(S(stream), logits, ld, rows, V, p, tokens_out));
}

// ---- logit rules ------------------------------------------------------------------------------------------------------
static int rules_values(const vh_logit_rules* r, int kmax, vh_mixtral::Rules* out, const char* what) {
    *out = vh_mixtral::Rules{};
    if (!r) return VH_OK;
    if (!std::isfinite(r->repetition_penalty) || !(r->repetition_penalty > 0.f))
        return fail(VH_E_ARG, "%s: repetition_penalty must be finite and > 0 (got %g)", what, (double)r->repetition_penalty);
    if (!std::isfinite(r->presence_penalty) || !std::isfinite(r->frequency_penalty))
        return fail(VH_E_ARG, "%s: presence_penalty and frequency_penalty must be finite", what);
    if (r->logprobs < -1 || r->logprobs > kmax) return fail(VH_E_ARG, "%s: logprobs %d outside [-1, %d]", what, r->logprobs, kmax);
    out->r = r->repetition_penalty; out->p = r->presence_penalty; out->f = r->frequency_penalty; out->K = r->logprobs;
    return VH_OK;
}
// validate the whole call, then write unit u's table (penalties only) and set its rules; nothing changes on a refusal
static int engine_rules(vh_mixtral* m, vh_mixtral::Unit& u, const vh_logit_rules* r, const int* ids, int n_prompt, int n_output,
                        const char* what) {
    if (!m->c.penalty_tables && m->c.max_logprobs <= 0)
        return fail(VH_E_ARG, "%s: the engine was created without penalty_tables and max_logprobs", what);
    if (r && r->logprobs >= 0 && m->c.max_logprobs <= 0) return fail(VH_E_ARG, "%s: logprobs need cfg.max_logprobs > 0", what);
    vh_mixtral::Rules v;
    const int rc = rules_values(r, m->c.max_logprobs > 0 ? m->c.max_logprobs : 0, &v, what);
    if (rc != VH_OK) return rc;
    if (v.pen() && !m->c.penalty_tables) return fail(VH_E_ARG, "%s: penalties need cfg.penalty_tables", what);
    if ((v.pen() || v.K >= 0) && m->c.vocab_n > 0)
        return fail(VH_E_ARG, "%s: penalties and logprobs need an unsharded LM head (vocab_n = %d of %d)", what, m->c.vocab_n, m->V);
    if (n_prompt < 0 || n_output < 0 || (!ids && n_prompt + (long)n_output > 0))
        return fail(VH_E_ARG, "%s: bad history (n_prompt %d, n_output %d)", what, n_prompt, n_output);
    const long n = (long)n_prompt + n_output;
    for (long i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= m->V) return fail(VH_E_ARG, "%s: id %d at %ld is outside [0, %d)", what, ids[i], i, m->V);
    // The table is rewritten (penalties) or cleared (it held a history and this request has no penalties).  It may still be read by
    // steps in flight on any stream of the engine's device: wait for that device, then write with blocking calls.
    if (v.pen() || (u.seen && u.seen_dirty)) {
        std::vector<unsigned> tab;
        if (v.pen()) {
            tab.assign((size_t)m->V, 0u);
            for (long i = 0; i < n_prompt; ++i) tab[ids[i]] |= 0x80000000u;
            for (long i = n_prompt; i < n; ++i) tab[ids[i]] += 1u;
        }
        int cur = -1;
        const bool hop = m->device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != m->device;
        if (hop && hipSetDevice(m->device) != hipSuccess) return fail(VH_E_HIP, "%s: cannot select device %d", what, m->device);
        const size_t bytes = (size_t)m->V * sizeof(unsigned);
        bool ok = hipDeviceSynchronize() == hipSuccess;
        ok = ok && (v.pen() ? hipMemcpy(u.seen, tab.data(), bytes, hipMemcpyHostToDevice) : hipMemset(u.seen, 0, bytes)) == hipSuccess;
        ok = ok && hipDeviceSynchronize() == hipSuccess;
        if (hop) (void)hipSetDevice(cur);
        if (!ok) return fail(VH_E_HIP, "%s: token table upload failed", what);
        u.seen_dirty = v.pen();
    }
    u.rules = v;
    return VH_OK;
}

int vh_mixtral_set_logit_rules(vh_mixtral_t* m, const vh_logit_rules* r, const int* ids, int n_prompt, int n_output) {
    if (!m) return fail(VH_E_ARG, "null engine");
    return engine_rules(m, m->units[0], r, ids, n_prompt, n_output, "vh_mixtral_set_logit_rules");
}

int vh_logit_rules_rows(const float* logits, long ld, int rows, int V, const vh_logit_rules* r, const uint32_t* seen, float* penalised_out,
                        const int* tokens, float* lp_tok, int* lp_top_id, float* lp_top, int K, void* stream) {
    const char* what = "vh_logit_rules_rows";
    if (!logits) return fail(VH_E_ARG, "%s: null pointer", what);
    if (rows < 1 || V < 1 || ld < 0) return fail(VH_E_SHAPE, "%s: rows %d, V %d, ld %ld", what, rows, V, ld);
    if (K < 0 || K > 20) return fail(VH_E_ARG, "%s: K %d outside [0, 20]", what, K);
    if (lp_tok && (!tokens || (K > 0 && (!lp_top_id || !lp_top)))) return fail(VH_E_ARG, "%s: logprobs need tokens and the top-K buffers", what);
    if (penalised_out && !r) return fail(VH_E_ARG, "%s: penalised_out needs rules", what);
    vh_mixtral::Rules v;
    vh_logit_rules rr = r ? *r : vh_logit_rules{1.f, 0.f, 0.f, -1};
    rr.logprobs = -1;
    const int rc = rules_values(&rr, 20, &v, what);
    if (rc != VH_OK) return rc;
    if (!penalised_out && !lp_tok) return VH_OK;
    const VhPenalty pen = seen ? VhPenalty{seen, v.r, v.f, v.p, 0} : VhPenalty{};
    return check_launch(what, vhk_logit_rules_rows(S(stream), logits, ld, rows, V, pen, penalised_out, tokens, lp_tok, lp_top_id, lp_top, K));
}

// a launcher returns non-zero when it REJECTS its arguments before launching (VH_E_SHAPE); a launch the runtime
// refused shows up in hipGetLastError (VH_E_HIP)
static int launch_failed(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VH_E_HIP, "%s: %s", what, hipGetErrorString(e));
    return fail(VH_E_SHAPE, "%s: launch rejected (shape / arguments)", what);
}
#define VH_TRY(expr, what)                             \
    do {                                               \
        if ((expr) != 0) return launch_failed(what);   \
    } while (0)

}  // extern "C" (reduce_rows below is a template)

// Row-parallel output under tensor parallelism (o_proj and the experts are RowParallel in the reference: vllm_file/mixtral.py:
// 405-414, 470-476): px += all-reduce(this rank's partial rows).  produce(h, part, ncols) enqueues the partial rows of output
// columns [h * ncols, (h + 1) * ncols) into part ([Sn][ncols]) on st.  overlap: two column halves, the all-reduce of half 0
// (comm stream) runs under the producer of half 1, then one add of both; otherwise all columns in one pass.
template <class Produce>
static int reduce_rows(vh_mixtral* m, hipStream_t st, int Sn, bool overlap, Produce&& produce) {
    const int H = m->H, H2 = H / 2;
    int rc;
    if (!overlap) {
        if ((rc = produce(0, m->ptmp, H)) != VH_OK) return rc;
        if (m->allreduce(m->ptmp, (long)Sn * H, st) != 0) return fail(VH_E_COMM, "all-reduce failed");
        VH_TRY(vhk_add(st, m->px, m->ptmp, (long)Sn * H), "add");
        return VH_OK;
    }
    for (int h = 0; h < 2; ++h) {
        float* part = m->ptmp + (size_t)h * Sn * H2;
        if ((rc = produce(h, part, H2)) != VH_OK) return rc;
        (void)hipEventRecord(m->ev_c[h], st);
        (void)hipStreamWaitEvent(m->cs, m->ev_c[h], 0);
        if (m->allreduce(part, (long)Sn * H2, m->cs) != 0) return fail(VH_E_COMM, "all-reduce failed");
        (void)hipEventRecord(m->ev_r[h], m->cs);
    }
    (void)hipStreamWaitEvent(st, m->ev_r[0], 0);
    (void)hipStreamWaitEvent(st, m->ev_r[1], 0);
    VH_TRY(vhk_add_halves(st, m->px, m->ptmp, m->ptmp + (size_t)Sn * H2, Sn, H), "add");
    return VH_OK;
}

// Weight-streaming MoE over n token rows, from the bf16 hi/lo planes (pxn_hi / lo) and top-2 ids (pids) that vhk_rmsnorm_route
// left: the rows are sorted by expert, gate|up runs one tall m-tile per expert (weights cross the fabric once) and emits the
// planes of h (ph_hi / lo), the down projection is K-split into `nslab` partial slabs of py that the combine adds.
struct MoeGemms {
    VhGemmPsArgs gate_up, down;   // launched by the caller (down: all H columns) through moe_gate_up / moe_down; W / W_up stay null:
    const VhExperts* x;           // the weights are the layer's experts, handed to the format's GEMM by moe_gate_up / moe_down_gemm
    int nslab;                    // slabs the combine adds (1 when the kernel picks the split ...
    const int* nslab_dev;         // ... and reports it here; null otherwise)
};
static int moe_gemms(vh_mixtral* m, hipStream_t st, const vh_mixtral_layer& w, int n, MoeGemms* p) {
    const int H = m->H, I = m->I, E = m->E;
    VH_TRY(vhk_moe_sort(st, m->pids, n, E, m->pgoff, m->pstok, m->psslot), "sort");
    *p = MoeGemms{};
    p->x = &m->X[&w - m->L.data()];
    VhGemmPsArgs &g = p->gate_up, &d = p->down;
    g.A_hi = m->pxn_hi; g.A_lo = m->pxn_lo; g.lda = H; g.a_rowidx = m->pstok;
    g.ldw = H; g.w_group_stride = (long)I * H;
    g.group_off = m->pgoff; g.ngroups = E;
    g.C_hi = m->ph_hi; g.C_lo = m->ph_lo; g.ldc_split = I; g.M = 2 * n; g.N = I; g.K = H; g.ksplit = 1;
    int ks = vh_tuning()->moe_ksplit;   // 1 .. 4 slabs, or -n: chosen by the kernel from the expert sizes (up to n)
    if (ks == 0) ks = 1;
    if (ks > 4) ks = 4;
    if (ks < -4) ks = -4;
    if (ks > (I >> 6)) ks = 1;
    d.A_hi = m->ph_hi; d.A_lo = m->ph_lo; d.lda = I;
    d.ldw = I; d.w_group_stride = (long)H * I;
    d.group_off = m->pgoff; d.ngroups = E;
    d.C = m->py; d.ldc = H; d.c_rowidx = m->psslot; d.M = 2 * n; d.N = H; d.K = I;
    d.ksplit = ks; d.c_split_stride = m->down_slab(H); d.nslab_out = m->pnslab;
    p->nslab = ks < 0 ? 1 : ks;
    p->nslab_dev = ks < 0 ? m->pnslab : nullptr;
    return VH_OK;
}
// The format's streaming GEMM on the layer's experts.  bf16: the weights go into the arguments; int8 / MXFP4: the specialised GEMM
// with that format's stagers (vhk_gemm_ps_i8 / _mxfp4), W / W_up null.  int8 scale groups are I (gate|up) and H (down) floats apart
static int moe_gate_up(hipStream_t st, const MoeGemms& p) {
    const VhExperts& x = *p.x;
    VhGemmPsArgs g = p.gate_up;
    switch (x.fmt) {
        case VH_EXPERTS_BF16: g.W = vh_as<uint16_t>(x.w1); g.W_up = vh_as<uint16_t>(x.w3); return vhk_gemm_ps(st, g);
        case VH_EXPERTS_I8: return vhk_gemm_ps_i8(st, g, VhPsI8{vh_as<int8_t>(x.w1), vh_as<int8_t>(x.w3), vh_as<float>(x.s1), vh_as<float>(x.s3), (long)g.N});
        case VH_EXPERTS_MXFP4: return vhk_gemm_ps_mxfp4(st, g, VhPsF4{vh_as<uint8_t>(x.w1), vh_as<uint8_t>(x.w3), vh_as<uint8_t>(x.s1), vh_as<uint8_t>(x.s3)});
    }
    return -1;
}
// the experts with w2 / s2 starting at row c0 of every expert's [H][I] down matrix (output column c0: a tensor-parallel half).  bf16 and
// int8 code rows are I elements, MXFP4 code rows I / 2 bytes; int8 has one scale per row, MXFP4 I / 32 scale bytes
static VhExperts w2_from_row(VhExperts x, int c0, long I) {
    switch (x.fmt) {
        case VH_EXPERTS_BF16: x.w2 = vh_as<uint16_t>(x.w2) + (size_t)c0 * I; break;
        case VH_EXPERTS_I8: x.w2 = vh_as<int8_t>(x.w2) + (size_t)c0 * I; x.s2 = vh_as<float>(x.s2) + c0; break;
        case VH_EXPERTS_MXFP4: x.w2 = vh_as<uint8_t>(x.w2) + (size_t)c0 * (I >> 1); x.s2 = vh_as<uint8_t>(x.s2) + (size_t)c0 * (I >> 5); break;
    }
    return x;
}
// down projection of output columns [c0, c0 + d.N) (d: p.down with N / C narrowed by the caller)
static int moe_down_gemm(hipStream_t st, const MoeGemms& p, const VhGemmPsArgs& d, int c0, int H) {
    const VhExperts x = w2_from_row(*p.x, c0, d.ldw);
    VhGemmPsArgs a = d;
    switch (x.fmt) {
        case VH_EXPERTS_BF16: a.W = vh_as<uint16_t>(x.w2); return vhk_gemm_ps(st, a);
        case VH_EXPERTS_I8: return vhk_gemm_ps_i8(st, a, VhPsI8{vh_as<int8_t>(x.w2), nullptr, vh_as<float>(x.s2), nullptr, (long)H});
        case VH_EXPERTS_MXFP4: return vhk_gemm_ps_mxfp4(st, a, VhPsF4{vh_as<uint8_t>(x.w2), nullptr, vh_as<uint8_t>(x.s2), nullptr});
    }
    return -1;
}
// the down projection of output columns [h * ncols, (h + 1) * ncols) into the slabs from py_half(h), then their
// routing-weighted sum into part ([n][ncols], zeroed first)
static int moe_down(vh_mixtral* m, hipStream_t st, const MoeGemms& p, int n, int h, int ncols,
                    float* part) {
    VhGemmPsArgs d = p.down;
    d.N = ncols; d.C = m->py_half(h); d.ldc = ncols; d.c_split_stride = m->down_slab(ncols);
    VH_TRY(moe_down_gemm(st, p, d, h * ncols, m->H), "down gemm");
    if (hipMemsetAsync(part, 0, (size_t)n * ncols * sizeof(float), st) != hipSuccess) return fail(VH_E_HIP, "memset failed");
    VH_TRY(vhk_moe_combine(st, part, d.C, m->pwts, n, ncols, p.nslab, d.c_split_stride, p.nslab_dev), "combine");
    return VH_OK;
}

// Vocab-sharded head: this rank's best per-block candidate (value, index; a 4-float key when sampled) goes into its slot of
// cand, the all-reduce fills the other world - 1 slots, and the world candidates replace the per-block ones for the select
static int exchange_candidates(vh_mixtral* m, hipStream_t st, float* blk_val, int* blk_idx, float* cand, int world, int keyed) {
    VH_TRY(vhk_dec_cand(st, blk_val, blk_idx, m->lm_grid, cand, m->c.tp_rank, world, keyed), "candidates");
    if (m->allreduce(cand, (keyed ? 4L : 2L) * world, st) != 0) return fail(VH_E_COMM, "all-reduce failed");
    VH_TRY(vhk_dec_cand_unpack(st, cand, world, blk_val, blk_idx, keyed), "candidates");
    return VH_OK;
}

// Final norm + LM head + token select for n units, in groups of up to VH_BMAX per pass over the table (a group of two or more: the
// batched LM-head kernel, one score row per member in samp_rows; a group of one: the single-row kernel on m->logits and lane 0).  Row b
// is x_in[b] (+ delta[b]; all null or all set), drawn with units[b]'s sampling parameters at its own draw index under its logit rules
// (penalties off: a null table, the kernels and launches of an engine without rules; on: folded into the head's per-block compare, or
// applied on load by the filter kernel; the select counts the token into the table); the token, the counters and the next embedding land
// in the unit.  Vocab-sharded head: every rank scores its rows, the (max, index) candidates travel through the all-reduce hook, every
// rank takes the same global argmax; kept scores are this rank's slice, zeros elsewhere.
struct HeadArgs {
    int mode = 1;                  // 1: a decode step (append, pos++); 0: the end of a prefill (first token, pos = set_pos[b])
    const int* set_pos = nullptr;  // mode 0: [n]
    int hist_rows = 1;             // rows of the score history a group of ONE keeps in m->logits (a larger group keeps one row per member)
    const VhXchg* cx = nullptr;    // fused MoE exchange the single-row LM head sums first (n = 1 only: the batched iteration has none)
    bool sharded = false;          // the per-block candidates are exchanged (vh_mixtral::head_sharded: the callers differ on loop-back)
    float* logits_out = nullptr;   // device fp32 [n][vocab], row b = the scores of x_in[b] (copied before the filter kernel's turn)
};
static int head(vh_mixtral* m, hipStream_t st, vh_mixtral::Unit* const* units, int n, const float* const* x_in, const float* const* delta,
                const HeadArgs& a) {
    const int H = m->H, V = m->V;
    const float eps = m->c.rms_eps;
    if (a.logits_out && a.sharded &&
        (hipMemsetAsync(m->samp_rows, 0, (size_t)VH_BMAX * V * sizeof(float), st) != hipSuccess ||
         hipMemsetAsync(m->logits, 0, (size_t)V * sizeof(float), st) != hipSuccess))
        return fail(VH_E_HIP, "memset failed");
    for (int g0 = 0; g0 < n; g0 += VH_BMAX) {
        const int gn = n - g0 < VH_BMAX ? n - g0 : VH_BMAX;
        const bool batched = gn >= 2;
        const int hist = batched ? 1 : a.hist_rows;
        VhDecBatchVec hv{};
        VhDecBatchHead hdp{};
        VhDecSampleJob sj{};
        VhDecLogprobJob lj{};
        VhPenalty pen[VH_BMAX] = {};
        bool filt[VH_BMAX] = {};
        float* row[VH_BMAX] = {};     // where member b's scores are kept
        hv.n = gn;
        sj.V = V; sj.hist_rows = hist;
        lj.V = V; lj.hist_rows = hist; lj.kmax = m->c.max_logprobs; lj.max_new = m->lp_rows();
        for (int b = 0; b < gn; ++b) {
            const vh_mixtral::Unit& u = *units[g0 + b];
            row[b] = batched ? m->samp_rows + (size_t)b * V : m->logits;
            hv.x_in[b] = x_in[g0 + b]; hv.delta[b] = delta[g0 + b];
            hdp.blk_val[b] = m->l_blk_val[b]; hdp.blk_idx[b] = m->l_blk_idx[b];
            hdp.ngen[b] = u.counters + 1;
            pen[b] = u.pen();
            filt[b] = sampling_filters(u.samp, V);   // top-k / top-p: greedy head, then the filter kernel on the kept row
            if (!filt[b]) { hdp.sample[b] = u.samp; hdp.pen[b] = pen[b]; }
            if (batched && (filt[b] || a.logits_out || u.rules.K >= 0)) hdp.logits[b] = row[b];
            if (u.rules.K >= 0) m->logprob_slot(lj, u, row[b]);
            if (filt[b]) {
                const int j = sj.n++;
                sj.logits[j] = row[b]; sj.ngen[j] = u.counters + 1;
                sj.blk_val[j] = m->l_blk_val[b]; sj.blk_idx[j] = m->l_blk_idx[b]; sj.sample[j] = u.samp;
                sj.pen[j] = pen[b];
            }
        }
        if (batched) {   // one pass over the table for the group: 97 us (four activation rows, always) against n x 70
            VH_TRY(vhk_decb_lmhead(st, hv, m->final_norm, eps, m->lm_head, m->Vn, H, hdp, m->lm_grid, m->v0), "batched lm_head");
        } else {
            VH_TRY(vhk_dec_lmhead(st, x_in[g0], delta[g0], m->final_norm, eps, m->lm_head, m->Vn, H, m->logits, m->l_blk_val[0],
                                  m->l_blk_idx[0], m->lm_grid, hdp.ngen[0], hist, m->v0, V, a.cx, &hdp.sample[0], &hdp.pen[0]), "lm_head");
        }
        if (a.logits_out)   // before the filter kernel's turn: it reads the rows, it does not change them
            for (int b = 0; b < gn; ++b)
                (void)hipMemcpyAsync(a.logits_out + (size_t)(g0 + b) * V, row[b], (size_t)V * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (sj.n > 0) VH_TRY(vhk_dec_sample(st, sj), "sample");   // one workgroup per filtered member of the group
        for (int b = 0; b < gn; ++b) {
            const vh_mixtral::Unit& u = *units[g0 + b];
            int nblk = filt[b] ? 1 : m->lm_grid;
            const int keyed = u.samp.T > 0.0 ? 1 : 0;   // sampled candidates travel as exact keys of their double scores
            if (a.sharded && !filt[b]) {
                nblk = m->cand_world();
                const int rc = exchange_candidates(m, st, m->l_blk_val[b], m->l_blk_idx[b], m->l_cand[b], nblk, keyed);
                if (rc != VH_OK) return rc;
            }
            VH_TRY(vhk_dec_select(st, m->l_blk_val[b], m->l_blk_idx[b], nblk, m->embed, H, V, u.xa, u.counters, u.counters + 1, u.tokens,
                                  m->c.max_new, a.mode, a.set_pos ? a.set_pos[g0 + b] : 0, keyed, const_cast<unsigned*>(pen[b].seen)), "select");
        }
        if (lj.n > 0) VH_TRY(vhk_dec_logprobs(st, lj), "logprobs");   // one workgroup per member of the group that asked for them
    }
    return VH_OK;
}
// The single-sequence form (a decode step or a one-segment prefill on unit u): n = 1, the engine's score history (logit_rows), the
// fused exchange of the step, and a loop-back communicator counts as a sharded head
static int head_one(vh_mixtral* m, hipStream_t st, vh_mixtral::Unit& u, const float* x_in, const float* delta, int mode, int set_pos,
                    const VhXchg* cx) {
    vh_mixtral::Unit* up = &u;
    HeadArgs a;
    a.mode = mode; a.set_pos = &set_pos; a.hist_rows = m->hist_rows(); a.cx = cx; a.sharded = m->head_sharded(/*loopback_counts=*/true);
    return head(m, st, &up, 1, &x_in, &delta, a);
}

// One pass over the weights for the rows of nseg segments, back to back in embeds, each on the unit it names.  One segment: unit 0 (the
// single-sequence engine, contiguous rows) or a slot.  Several: distinct slots, addressed in place — everything row-wise runs on all
// Sn rows at once; RoPE + KV write and attention take the segment descriptors, the head runs on the list of units.
// dec: the segment is ONE DECODE STEP of its unit (a mixed pass, vh_mixtral_seq_step): len 1 at pos0 = the unit's position, its row is the
// embedding the last select left in the unit's xa, its counters go on, the head runs in mode 1.  Decode segments follow the prefill ones.
struct PfSeg { int unit, len, pos0; int dec = 0; };
static int prefill_enqueue(vh_mixtral* m, const float* embeds, const PfSeg* sg, int nseg, float* logits_out, float* hidden_dbg,
                           hipStream_t st);
// The host mirrors of a prefill move here: a pass that was enqueued whole advances its units; one that was not loses its slots (a
// slot is then poisoned until freed; unit 0 is not — its next prefill starts over anyway).  A one-segment pass clears the flag of its
// unit once it is under way (prefill_enqueue).
static int prefill_impl(vh_mixtral* m, const float* embeds, const PfSeg* sg, int nseg, float* logits_out, float* hidden_dbg,
                        hipStream_t st) {
    const int rc = prefill_enqueue(m, embeds, sg, nseg, logits_out, hidden_dbg, st);
    for (int i = 0; i < nseg; ++i) {
        vh_mixtral::Unit& u = m->units[sg[i].unit];
        if (rc == VH_OK) u.host_pos = sg[i].pos0 + sg[i].len;
        else if (sg[i].unit > 0) u.poisoned = 1;
    }
    return rc;
}
static int prefill_enqueue(vh_mixtral* m, const float* embeds, const PfSeg* sg, int nseg, float* logits_out, float* hidden_dbg,
                           hipStream_t st) {
    int Sn = 0, kmax = 0, npf = 0, Spf = 0, kmax_pf = 0;
    for (int i = 0; i < nseg; ++i) {
        if (sg[i].len < 1) return fail(VH_E_SHAPE, "prefill length %d outside [1,%d]", sg[i].len, m->c.max_prefill);
        if (sg[i].pos0 < 0 || sg[i].pos0 + sg[i].len >= m->c.max_ctx) return fail(VH_E_SHAPE, "prefill exceeds KV capacity %d", m->c.max_ctx);
        if (sg[i].dec ? sg[i].len != 1 : npf != i) return fail(VH_E_ARG, "mixed pass: decode segments are single rows behind the prefill segments");
        Sn += sg[i].len;
        if (sg[i].pos0 + sg[i].len > kmax) kmax = sg[i].pos0 + sg[i].len;
        if (!sg[i].dec) { ++npf; Spf += sg[i].len; kmax_pf = kmax; }
    }
    if (Sn < 1 || Sn > m->c.max_prefill) return fail(VH_E_SHAPE, "prefill length %d outside [1,%d]", Sn, m->c.max_prefill);
    const int ndec = nseg - npf;
    const bool multi = nseg > 1 || ndec > 0;
    const int pos0 = sg[0].pos0;
    vh_mixtral::Unit& u0 = m->units[sg[0].unit];   // the unit of a one-segment pass
    const int H = m->H, nq = m->nq, nkv = m->nkv, hd = m->hd, KO = nq * hd;
    const bool tp = m->c.tp_world > 1 || vh_tuning()->force_allreduce;
    const float scale = 1.0f / sqrtf((float)hd);
    int rc;
    if (Spf > 0 && hipMemcpyAsync(m->px, embeds, (size_t)Spf * H * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return fail(VH_E_HIP, "prefill: embed copy failed");
    for (int i = npf; i < nseg; ++i)   // a decode member's row: the embedding its last select left in xa (gathered before any head rewrites it)
        if (hipMemcpyAsync(m->px + (size_t)(Spf + i - npf) * H, m->units[sg[i].unit].xa, (size_t)H * sizeof(float), hipMemcpyDeviceToDevice,
                           st) != hipSuccess)
            return fail(VH_E_HIP, "mixed pass: row gather failed");
    if (multi) {
        // the descriptors go up once, before layer 0, from storage that outlives the copy; every listed slot starts as the unit of a
        // one-segment pass does below (counters 1-3 zeroed)
        m->segs_host.resize(nseg);
        int row0 = 0;
        for (int i = 0; i < nseg; ++i) {
            const vh_mixtral::Unit& u = m->units[sg[i].unit];
            m->segs_host[i] = VhSeg{row0, sg[i].len, sg[i].pos0, 0, u.table};
            row0 += sg[i].len;
            if (!sg[i].dec && hipMemsetAsync(u.counters + 1, 0, 3 * sizeof(int), st) != hipSuccess) return fail(VH_E_HIP, "memset failed");
        }
        if (hipMemcpyAsync(m->seq_segs, m->segs_host.data(), (size_t)nseg * sizeof(VhSeg), hipMemcpyHostToDevice, st) != hipSuccess)
            return fail(VH_E_HIP, "prefill: segment descriptor upload failed");
    } else {
        if (hipMemsetAsync(u0.counters + 1, 0, 3 * sizeof(int), st) != hipSuccess) return fail(VH_E_HIP, "memset failed");
        u0.poisoned = 0;
    }
    if (m->c.vocab_n > 0 && m->c.tp_world > 1 &&
        hipMemsetAsync(m->logits, 0, (size_t)m->hist_rows() * m->V * sizeof(float), st) != hipSuccess)
        return fail(VH_E_HIP, "memset failed");   // vocab-sharded head: a kept score row holds THIS rank's slice, zeros elsewhere
    // overlapped tensor-parallel prefill: needs a collective that takes a stream, and halves that stay 16-byte rows
    const bool overlap = tp && vh_tuning()->tp_overlap != 0 && m->stream_capable() && ((H / 2) % 4) == 0 && Sn >= 16;
    if (overlap) {
        if (m->ensure_comm_stream() != 0) return fail(VH_E_HIP, "prefill: comm stream creation failed");
        // the comm stream starts behind everything already queued on the compute stream
        (void)hipEventRecord(m->ev_c[0], st);
        (void)hipStreamWaitEvent(m->cs, m->ev_c[0], 0);
    }

    // py holds 8 * max_prefill * H floats: K-split slabs of the projections (and of the MoE down projection later)
    int qkv_slabs = (int)((8L * H) / m->nqkv);
    if (qkv_slabs > 4) qkv_slabs = 4;
    const bool stream_attn = vh_tuning()->prefill_attn_gemm == 0 && qkv_slabs >= 1 && (H % 64) == 0 && (KO % 64) == 0 &&
                             H <= 4096 && (m->nqkv % 4) == 0;
    // (r03) K-split slabs are summed by the norm kernel that consumes the rows (VhRowUpdate) on the single-rank path;
    // vh_tune("prefill_fuse_rows", 0) restores the separate slab-sum / combine launches
    const bool fuse_rows = !tp && vh_tuning()->prefill_fuse_rows != 0 && stream_attn;
    const bool attn_planes = stream_attn && vh_tuning()->prefill_fuse_rows != 0 && (hd == 64 || hd == 128);
    // (r06) one-shot prefills whose attention is the flash kernel get K / V as MFMA-ready tile images from the RoPE pass
    bool use_img = false;
    if (!multi && stream_attn && pos0 == 0 && m->kv_img && (Sn + 63) / 64 <= m->img_tiles && vh_tuning()->attn_img != 0) {
        VhAttnArgs q{};
        q.Sq = Sn; q.Sk = Sn; q.d = hd; q.Hq = nq; q.Hkv = nkv; q.B = 1; q.causal = 1;
        use_img = vhk_attn_fa_applies(q) != 0;
    }
    // the single rows of a mixed pass: the split-KV row kernels (head_dim 128, up to 4 query heads per KV head: the geometry they are
    // written for), with py - idle between the RoPE pass and the O projection - as their scratch; vh_tune("step_attn", 0) or another
    // geometry: 1-row segments of the segment attention
    const bool row_attn = ndec > 0 && vh_tuning()->step_attn != 0 && hd == 128 && nq % nkv == 0 && nq / nkv <= 4;
    const int nsa = row_attn ? npf : nseg, Ssa = row_attn ? Spf : Sn, ksa = row_attn ? kmax_pf : kmax;   // what the segment attention takes
    bool combine_pending = false;
    int pend_nslab = 1;
    const int* pend_nslab_dev = nullptr;
    for (int l = 0; l < m->c.n_layers; ++l) {
        const vh_mixtral_layer& w = m->L[l];
        float* kc = m->kcache + (size_t)l * nkv * m->c.max_ctx * hd;
        float* vc = m->vcache + (size_t)l * nkv * m->c.max_ctx * hd;
        // ---- attention norm + QKV + RoPE
        if (stream_attn) {
            // weight-streaming projections (vh_gemm_ps.hip): the norm emits the bf16 hi/lo planes, the 35 row tiles of
            // S = 552 run as 3 m-tiles per 256 weight rows and the kernel picks a K split that fills the CUs
            // (72 QKV tiles x 3 slabs); the partial slabs are summed by the consumer (RoPE / KV write)
            // (r03) the previous layer's expert outputs are still K-split slabs in py: this norm applies the routing-weighted
            // sum to the residual rows first (VhRowUpdate), so no combine kernel runs between the layers
            const VhRowUpdate cu{m->py, (long)H, m->down_slab(H), pend_nslab_dev, pend_nslab, m->pwts};
            VH_TRY(vhk_rmsnorm_route(st, m->px, nullptr, m->pxn_hi, m->pxn_lo, w.attn_norm, Sn, H, m->c.rms_eps, nullptr, 0,
                                     nullptr, nullptr, combine_pending ? &cu : nullptr), "rmsnorm");
            if (combine_pending && hidden_dbg)
                (void)hipMemcpyAsync(hidden_dbg + (size_t)(l - 1) * Sn * H, m->px, (size_t)Sn * H * sizeof(float),
                               hipMemcpyDeviceToDevice, st);
            combine_pending = false;
            VhGemmPsArgs g{};
            g.A_hi = m->pxn_hi; g.A_lo = m->pxn_lo; g.lda = H;
            g.W = w.wqkv; g.ldw = H; g.C = m->py; g.ldc = m->nqkv; g.M = Sn; g.N = m->nqkv; g.K = H;
            g.ksplit = -qkv_slabs; g.c_split_stride = m->proj_slab(m->nqkv); g.nslab_out = m->pnslab + 1;
            VH_TRY(vhk_gemm_ps(st, g), "qkv gemm");
            if (use_img)   // one-shot prefill under the flash kernel: RoPE + cache write + the K / V tile images in one pass
                VH_TRY(vhk_rope_kv_img(st, m->py, m->nqkv, m->pq, kc, vc, m->rope_cos, m->rope_sin, Sn, nq, nkv, m->c.max_ctx,
                                       u0.table, m->pnslab + 1, g.c_split_stride, m->kv_img, m->img_tiles), "rope + images");
            else if (multi)   // all segments in one launch: row -> (segment, position, page row) from the descriptors
                VH_TRY(vhk_rope_kv_segs(st, m->py, m->nqkv, m->pq, kc, vc, m->rope_cos, m->rope_sin, Sn, m->seq_segs, nseg, nq, nkv,
                                        m->c.max_ctx, m->pnslab + 1, g.c_split_stride), "rope");
            else
                VH_TRY(vhk_rope_kv(st, m->py, m->nqkv, m->pq, kc, vc, m->rope_cos, m->rope_sin, Sn, pos0, nq, nkv,
                                   m->c.max_ctx, u0.table, m->pnslab + 1, g.c_split_stride), "rope");
        } else {
            VH_TRY(vhk_rmsnorm(st, m->px, m->pxn, w.attn_norm, Sn, H, m->c.rms_eps), "rmsnorm");
            VhGemmArgs g{};
            g.A = m->pxn; g.lda = H; g.a_rows = Sn; g.nseg = 1; g.seglen = H;
            g.W = w.wqkv; g.ldw = H; g.C = m->pqkv; g.ldc = m->nqkv; g.M = Sn; g.N = m->nqkv; g.K = H;
            VH_TRY(vhk_gemm(st, g), "qkv gemm");
            if (multi)
                VH_TRY(vhk_rope_kv_segs(st, m->pqkv, m->nqkv, m->pq, kc, vc, m->rope_cos, m->rope_sin, Sn, m->seq_segs, nseg, nq, nkv,
                                        m->c.max_ctx, nullptr, 0), "rope");
            else
                VH_TRY(vhk_rope_kv(st, m->pqkv, m->nqkv, m->pq, kc, vc, m->rope_cos, m->rope_sin, Sn, pos0, nq, nkv,
                                   m->c.max_ctx, u0.table, nullptr, 0), "rope");
        }
        // ---- attention
        VhAttnArgs a{};
        a.Q = m->pq; a.ldq = KO; a.hsq = hd;
        a.K = kc; a.ldk = hd; a.hsk = (long)m->c.max_ctx * hd;
        a.V = vc; a.ldv = hd; a.hsv = (long)m->c.max_ctx * hd;
        a.O = m->pattn; a.ldo = KO;
        a.B = 1; a.Hq = nq; a.Hkv = nkv; a.Sq = Sn; a.Sk = pos0 + Sn; a.d = hd;
        a.causal = 1; a.q_off = pos0; a.klen = pos0 + Sn; a.chunk = 0; a.left = -1; a.scale = scale;
        a.ktable = u0.table; a.kv_rows = m->c.max_ctx;
        if (multi) {   // every segment against its own sequence's pages, one call
            a.segs = m->seq_segs; a.segs_host = m->segs_host.data(); a.nseg = nsa;
            a.Sq = Ssa; a.Sk = ksa; a.klen = ksa; a.q_off = 0; a.ktable = nullptr;
        }
        if (use_img) { a.kv_img = m->kv_img; a.img_tiles = m->img_tiles; }
        if (attn_planes) { a.O = nullptr; a.O_hi = m->ph_hi; a.O_lo = m->ph_lo; a.ldo_split = KO; }
        if (nsa > 0) VH_TRY(vhk_attn(st, a), "attention");
        if (row_attn)
            VH_TRY(vhk_attn_rows(st, m->pq, KO, m->seq_segs + npf, m->segs_host.data() + npf, ndec, kc, vc, nq, nkv, m->c.max_ctx, scale,
                                 m->py, (size_t)4 * m->down_slab(H), attn_planes ? nullptr : m->pattn, attn_planes ? m->ph_hi : nullptr,
                                 attn_planes ? m->ph_lo : nullptr, KO), "row attention");
        // ---- O projection
        bool o_pending = false;
        if (stream_attn) {
            // on the streaming kernel: planes of the attention output (written by the attention kernel itself when it is the
            // direct-operand one), K-split slabs, slab sum fused into the FFN norm (or feeding the all-reduce under tensor
            // parallelism)
            if (!attn_planes) VH_TRY(vhk_split_planes(st, m->pattn, KO, m->ph_hi, m->ph_lo, KO, Sn, KO), "split planes");
            VhGemmPsArgs g{};
            g.A_hi = m->ph_hi; g.A_lo = m->ph_lo; g.lda = KO;
            g.ldw = KO; g.M = Sn; g.K = KO; g.ksplit = -8;
            // output columns [h * ncols, (h + 1) * ncols) as K-split slabs from py_half(h), then (part != null) their sum into part
            auto o_slabs = [&](int h, float* part, int ncols) -> int {
                g.W = w.wo + (size_t)h * ncols * KO; g.N = ncols; g.C = m->py_half(h); g.ldc = ncols;
                g.c_split_stride = m->proj_slab(ncols); g.nslab_out = m->pnslab + 2 + h;
                VH_TRY(vhk_gemm_ps(st, g), "o gemm");
                if (part) VH_TRY(vhk_sum_slabs(st, part, ncols, g.C, ncols, Sn, ncols, g.nslab_out, 1, g.c_split_stride, 0), "slab sum");
                return VH_OK;
            };
            if (tp) {
                if ((rc = reduce_rows(m, st, Sn, overlap, o_slabs)) != VH_OK) return rc;
            } else {
                if ((rc = o_slabs(0, nullptr, H)) != VH_OK) return rc;
                if (fuse_rows) o_pending = true;   // summed into px by the FFN norm below
                else VH_TRY(vhk_sum_slabs(st, m->px, H, m->py, H, Sn, H, m->pnslab + 2, 1, m->proj_slab(H), 1), "slab sum");
            }
        } else {
            VhGemmArgs g{};
            g.A = m->pattn; g.lda = KO; g.a_rows = Sn; g.nseg = 1; g.seglen = KO;
            g.W = w.wo; g.ldw = KO; g.M = Sn; g.N = H; g.K = KO;
            if (tp) {
                rc = reduce_rows(m, st, Sn, overlap, [&](int h, float* part, int ncols) -> int {
                    g.W = w.wo + (size_t)h * ncols * KO; g.N = ncols; g.C = part; g.ldc = ncols;
                    VH_TRY(vhk_gemm(st, g), "o gemm");
                    return VH_OK;
                });
                if (rc != VH_OK) return rc;
            } else {
                g.C = m->px; g.ldc = H; g.resid = m->px; g.ldr = H;
                VH_TRY(vhk_gemm(st, g), "o gemm");
            }
        }
        // ---- experts
        const VhRowUpdate ou{m->py, (long)H, m->proj_slab(H), m->pnslab + 2, 1, nullptr};     // the O projection's slabs
        VH_TRY(vhk_rmsnorm_route(st, m->px, nullptr, m->pxn_hi, m->pxn_lo, w.ffn_norm, Sn, H, m->c.rms_eps, w.wrouter,
                                 m->E, m->pids, m->pwts, o_pending ? &ou : nullptr), "rmsnorm + route");
        MoeGemms moe;
        if ((rc = moe_gemms(m, st, w, Sn, &moe)) != VH_OK) return rc;
        const bool prof = m->prof_stride < 0 && (l % -m->prof_stride) == 0 && m->prof_used + 2 <= m->prof_ev.size();
        if (prof) (void)hipEventRecord(m->prof_ev[m->prof_used], st);
        VH_TRY(moe_gate_up(st, moe), "gate/up gemm");
        if (prof) { (void)hipEventRecord(m->prof_ev[m->prof_used + 1], st); m->prof_used += 2; }
        if (tp) {
            rc = reduce_rows(m, st, Sn, overlap,
                             [&](int h, float* part, int ncols) { return moe_down(m, st, moe, Sn, h, ncols, part); });
            if (rc != VH_OK) return rc;
        } else {
            VH_TRY(moe_down_gemm(st, moe, moe.down, 0, H), "down gemm");
            if (fuse_rows && l + 1 < m->c.n_layers) {
                combine_pending = true;             // applied by the next layer's attention norm
                pend_nslab = moe.nslab; pend_nslab_dev = moe.nslab_dev;
            } else {
                VH_TRY(vhk_moe_combine(st, m->px, m->py, m->pwts, Sn, H, moe.nslab, m->down_slab(H), moe.nslab_dev), "combine");
            }
        }
        // ---- debug copies (a pending combine: the next layer's attention norm applies it, then copies this layer's rows)
        if (m->route_dbg)
            (void)hipMemcpyAsync(m->route_dbg + (size_t)l * 2 * Sn, m->pids, (size_t)2 * Sn * sizeof(int),
                           hipMemcpyDeviceToDevice, st);
        if (hidden_dbg && !combine_pending)
            (void)hipMemcpyAsync(hidden_dbg + (size_t)l * Sn * H, m->px, (size_t)Sn * H * sizeof(float),
                           hipMemcpyDeviceToDevice, st);
    }
    // logits of the last position only (the reference computes all S rows and uses the last:
    // vita_mixtral.py:171-172 + HF greedy argmax(logits[:, -1]))
    if (multi) {
        // the first token of every segment: final norm + LM head + select on the segments' last rows, each with its slot's sampling,
        // counters and next-embedding row (the head of a batched decode iteration)
        std::vector<vh_mixtral::Unit*> us(nseg);
        std::vector<int> set_pos(nseg);
        std::vector<const float*> xin(nseg), dl(nseg, nullptr);
        for (int i = 0; i < nseg; ++i) {
            us[i] = &m->units[sg[i].unit]; set_pos[i] = sg[i].pos0 + sg[i].len;
            xin[i] = m->px + (size_t)(m->segs_host[i].row0 + sg[i].len - 1) * H;
        }
        HeadArgs ha;
        ha.mode = 0; ha.set_pos = set_pos.data(); ha.sharded = m->head_sharded(/*loopback_counts=*/false); ha.logits_out = logits_out;
        if (npf > 0 && (rc = head(m, st, us.data(), npf, xin.data(), dl.data(), ha)) != VH_OK) return rc;
        if (ndec > 0) {   // the decode members of a mixed pass: a decode step's head (append, pos + 1, counters and draw index go on)
            HeadArgs hb;
            hb.sharded = ha.sharded; hb.logits_out = logits_out ? logits_out + (size_t)npf * m->V : nullptr;
            if ((rc = head(m, st, us.data() + npf, ndec, xin.data() + npf, dl.data() + npf, hb)) != VH_OK) return rc;
        }
    } else {
        if ((rc = head_one(m, st, u0, m->px + (size_t)(Sn - 1) * H, nullptr, /*mode=*/0, /*set_pos=*/pos0 + Sn, nullptr)) != VH_OK) return rc;
        if (logits_out)
            (void)hipMemcpyAsync(logits_out, m->logits, (size_t)m->V * sizeof(float), hipMemcpyDeviceToDevice, st);
    }
    hipError_t e = hipGetLastError();          // also what an event / copy enqueue above ((void) calls) left behind
    if (e != hipSuccess) return fail(VH_E_HIP, "prefill: %s", hipGetErrorString(e));
    return VH_OK;
}

static int api_num_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        n = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    }
    return n;
}

extern "C" {

int vh_encoder_layer(const vh_encoder_layer_args* a, void* stream) {
    if (!a || !a->x || !a->h_in || !a->qkv_w || !a->proj_w || !a->n2_w || !a->fc1_w || !a->fc2_w || !a->qkv || !a->attn ||
        !a->hmid || !a->mid)
        return fail(VH_E_ARG, "vh_encoder_layer: null pointer");
    const int M = a->M, Cw = a->C, F = a->F;
    if (M < 1 || a->B < 1 || M % a->B != 0 || a->heads < 1 || Cw % a->heads != 0 || Cw % 64 != 0 || F % 64 != 0)
        return fail(VH_E_SHAPE, "vh_encoder_layer: M %d B %d C %d F %d heads %d", M, a->B, Cw, F, a->heads);
    const int d = Cw / a->heads, Sq = M / a->B;
    if (d != 64 && d != 128) return fail(VH_E_SHAPE, "vh_encoder_layer: head_dim %d (64 or 128)", d);
    if (a->P && (!a->bias_u || !a->bias_v)) return fail(VH_E_ARG, "vh_encoder_layer: rel-pos needs bias_u / bias_v");
    if (a->h_out && !a->next_w) return fail(VH_E_ARG, "vh_encoder_layer: h_out without next_w");
    hipStream_t st = S(stream);
    auto lin = [&](const float* A, int K, const uint16_t* W, int N, const float* bias, int act, const float* scale, const float* resid,
                   float* Cout, const float* lw, const float* lb, float* lout) {
        VhGemmArgs g{};
        g.A = A; g.lda = K; g.a_rows = M; g.nseg = 1; g.seglen = K;
        g.W = W; g.ldw = K; g.C = Cout; g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = act;
        g.bias = bias; g.scale = scale; g.resid = resid; g.ldr = N;
        g.ws = a->ws; g.ws_bytes = a->ws_bytes; g.ksplit = a->ws ? 0 : 1;
        g.ln_w = lw; g.ln_b = lb; g.ln_eps = a->eps; g.ln_out = lout; g.ld_ln = N;
        return vhk_gemm(st, g);
    };
    // ---- planes = 1: the four Linears on the streaming GEMM, operands as bf16 hi/lo planes (see include/vita_hip.h) -------------------
    const bool planes = a->planes != 0;
    if (planes && (a->P || !a->ws || a->ws_bytes < (size_t)M * Cw * sizeof(float)))
        return fail(VH_E_ARG, "vh_encoder_layer: planes = 1 needs ws >= 4 M C bytes and no rel-pos operand");
    auto pl_hi = [&](const void* base) { return reinterpret_cast<uint16_t*>(const_cast<void*>(base)); };
    auto pl_lo = [&](const void* base, long cols) { return reinterpret_cast<uint16_t*>(const_cast<void*>(base)) + (size_t)M * cols; };
    // K split of a Linear whose one-pass tiling cannot fill half the chip (N = C: 4 n-tiles): 2 .. 4 by depth, bounded by ws
    auto ks_for = [&](int N, int K) {
        const long nrt = (M + 15) >> 4, NT = (N + 255) / 256;
        if (((nrt + 2) / 3) * NT * 2 >= api_num_cus()) return 1;
        int ks = K / 1024 + 1;
        ks = ks < 2 ? 2 : (ks > 4 ? 4 : ks);
        while (ks > 1 && ((size_t)ks * M * N * sizeof(float) > a->ws_bytes || ks > (K >> 6))) --ks;
        return ks;
    };
    // out = A W^T on planes: raw partial sums into ws (ks slabs), or the finished rows (bias, act) as fp32 / as planes
    auto lin_ps = [&](const void* A, int K, const uint16_t* W, int N, const float* bias, int act, float* Cout, void* Cplanes, int ks) {
        VhGemmPsArgs g{};
        g.A_hi = pl_hi(A); g.A_lo = pl_lo(A, K); g.lda = K;
        g.W = W; g.ldw = K; g.M = M; g.N = N; g.K = K;
        if (ks >= 1 && !Cout && !Cplanes) { g.C = a->ws; g.ldc = N; g.ksplit = ks; g.c_split_stride = (long)M * N; }
        else { g.C = Cout; g.ldc = N; g.bias = bias; g.act = act; g.ksplit = 1;
               if (Cplanes) { g.C_hi = pl_hi(Cplanes); g.C_lo = pl_lo(Cplanes, N); g.ldc_split = N; } }
        return vhk_gemm_ps(st, g);
    };
    // x += scale * (sum of the ks slabs + bias); then LN(x; lw, lb) as planes into lout (nullable)
    auto reduce_into_x = [&](int N, int ks, const float* bias, const float* scale, const float* lw, const float* lb, void* lout) {
        VhGemmArgs g{};
        g.ws = a->ws; g.ws_bytes = a->ws_bytes; g.M = M; g.N = N; g.C = a->x; g.ldc = N;
        g.bias = bias; g.scale = scale; g.resid = a->x; g.ldr = N; g.act = VH_ACT_NONE;
        if (lout) { g.ln_w = lw; g.ln_b = lb; g.ln_eps = a->eps; g.ln_hi = pl_hi(lout); g.ln_lo = pl_lo(lout, N); g.ld_ln_split = N; }
        return vhk_gemm_reduce(st, g, ks);
    };
    if (planes) VH_TRY(lin_ps(a->h_in, Cw, a->qkv_w, 3 * Cw, a->qkv_b, VH_ACT_NONE, a->qkv, nullptr, 1), "encoder qkv (planes)");
    else
    VH_TRY(lin(a->h_in, Cw, a->qkv_w, 3 * Cw, a->qkv_b, VH_ACT_NONE, nullptr, nullptr, a->qkv, nullptr, nullptr, nullptr), "encoder qkv");
    {
        VhAttnArgs g{};
        g.Q = a->qkv; g.K = a->qkv + Cw; g.V = a->qkv + 2 * Cw;
        g.ldq = g.ldk = g.ldv = 3L * Cw; g.hsq = g.hsk = g.hsv = d;
        g.bsq = g.bsk = (long)Sq * 3 * Cw; g.bso = (long)Sq * Cw;
        if (planes) { g.O = nullptr; g.O_hi = pl_hi(a->attn); g.O_lo = pl_lo(a->attn, Cw); g.ldo_split = Cw; }
        else g.O = a->attn;
        g.ldo = Cw;
        g.B = a->B; g.Hq = g.Hkv = a->heads; g.Sq = g.Sk = Sq; g.d = d;
        g.klen = (a->klen >= 0 && a->klen < Sq) ? a->klen : Sq; g.chunk = a->chunk; g.left = a->left;
        g.scale = 1.0f / sqrtf((float)d);
        g.P = a->P; g.ldp = a->ldp; g.hsp = d; g.bias_u = a->bias_u; g.bias_v = a->bias_v;
        g.klens = a->klens;
        const int rc = vhk_attn(st, g);
        if (rc == -2) return fail(VH_E_ARG, "vh_encoder_layer: klens needs the fp32 direct attention kernel (rel-pos, a chunk mask or attn_impl 2)");
        VH_TRY(rc, "encoder attention");
    }
    if (planes) {
        const int ks1 = ks_for(Cw, Cw), ks2 = ks_for(Cw, F);
        VH_TRY(lin_ps(a->attn, Cw, a->proj_w, Cw, nullptr, VH_ACT_NONE, nullptr, nullptr, ks1), "encoder proj (planes)");
        VH_TRY(reduce_into_x(Cw, ks1, a->proj_b, a->ls1, a->n2_w, a->n2_b, a->hmid), "encoder proj reducer");
        VH_TRY(lin_ps(a->hmid, Cw, a->fc1_w, F, a->fc1_b, a->act, nullptr, a->mid, 1), "encoder fc1 (planes)");
        VH_TRY(lin_ps(a->mid, F, a->fc2_w, Cw, nullptr, VH_ACT_NONE, nullptr, nullptr, ks2), "encoder fc2 (planes)");
        VH_TRY(reduce_into_x(Cw, ks2, a->fc2_b, a->ls2, a->next_w, a->next_b, a->h_out), "encoder fc2 reducer");
        hipError_t e2 = hipGetLastError();
        if (e2 != hipSuccess) return fail(VH_E_HIP, "vh_encoder_layer: %s", hipGetErrorString(e2));
        return VH_OK;
    }
    VH_TRY(lin(a->attn, Cw, a->proj_w, Cw, a->proj_b, VH_ACT_NONE, a->ls1, a->x, a->x, a->n2_w, a->n2_b, a->hmid), "encoder proj");
    VH_TRY(lin(a->hmid, Cw, a->fc1_w, F, a->fc1_b, a->act, nullptr, nullptr, a->mid, nullptr, nullptr, nullptr), "encoder fc1");
    VH_TRY(lin(a->mid, F, a->fc2_w, Cw, a->fc2_b, VH_ACT_NONE, a->ls2, a->x, a->x, a->h_out ? a->next_w : nullptr, a->next_b,
               a->h_out), "encoder fc2");
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VH_E_HIP, "vh_encoder_layer: %s", hipGetErrorString(e));
    return VH_OK;
}

int vh_mixtral_prefill(vh_mixtral_t* m, const float* embeds, int Sn, int pos0, float* logits_out, float* hidden_dbg,
                       void* stream) {
    if (!m || !embeds) return fail(VH_E_ARG, "vh_mixtral_prefill: null pointer");
    if (m->live_seqs() > 0) return fail(VH_E_ARG, "vh_mixtral_prefill: sequences own pages of the KV pool (free them or reset)");
    if (m->pages_in_use())
        return fail(VH_E_ARG, "%s: pages of the KV pool are held (vh_mixtral_seq_hold_prefix; serving: the prefix cache): release them "
                              "(vh_mixtral_pages_release / reset_prefix_cache) or reset", "vh_mixtral_prefill");
    const PfSeg one{0, Sn, pos0};
    return prefill_impl(m, embeds, &one, 1, logits_out, hidden_dbg, S(stream));
}

int vh_mixtral_decode_schedule(const vh_mixtral_t* m) { return m ? m->schedule_state : -1; }

// Attention block of a decode layer as one fused launch (k_dec_ablk) or as three (QKV, attention, O projection): vh_tune("dec_fused").
static bool fused_wanted(const vh_mixtral* m) {
    const int want = vh_tuning()->dec_fused;        // -1 auto, 0 never, 1 wherever the kernel has an instantiation
    if (want == 0) return false;
    return vhk_dec_ablk_supported(m->H, m->nq, m->nkv) != 0;
}

// One decode step of unit u (all layers + LM head + token select) enqueued on st.  Returns VH_OK or an error code; the host
// mirrors move in step_unit, only after the step was enqueued without error.
// Three launches per layer: the attention block (k_dec_ablk: fused QKV -> attention -> O projection; three launches with
// vh_tune("dec_fused", 0)), gate|up, down.
// Tensor parallel over the library's IPC transport: the two all-reduces of a layer are either FUSED into the kernels around
// them (VhXchg, vh_kernels.h: the O-projection items / the MoE down projection push their partial outputs straight into the
// peers' receive slots, the first blocks of the next launch — gate|up, the next layer's attention block, the LM head — sum the
// slots in rank order and every block of it waits for that sum behind its own weight loads: "all-reduce over xGMI overlapped
// with the expert GEMMs", web_demo/vllm_tools/vllm_file/mixtral.py:405-414,470-476; no launch per exchange) — the form the ranks
// vote for when each owns its device — or one small all-reduce kernel per exchange (ranks sharing a device: a waiting consumer
// grid would hold the CUs a peer's producer needs).
static int decode_one_step(vh_mixtral* m, vh_mixtral::Unit& u, hipStream_t st) {
    const int H = m->H, I = m->I, nq = m->nq, nkv = m->nkv, hd = m->hd;
    const float scale = 1.0f / sqrtf((float)hd);
    const float eps = m->c.rms_eps;
    const bool fuse = m->comm != nullptr && m->exchanges() && vh_tuning()->tp_fuse != 0 && (H % 2) == 0 &&
                      (size_t)H <= vh_comm_capacity(m->comm) && H <= 32768 && !vh_tuning()->force_allreduce;
    // Engine processes SHARING a device (ranks of the one-device tests, duplex replicas on one GPU) keep the three launches: a launch whose
    // blocks wait for other blocks is safe only while nobody else's waiting blocks can occupy the slots its producers need — blocks are
    // dispatched in index order PER XCD, so rank A's O blocks can fill one XCD while A's attention blocks queue on another behind rank B's
    // O blocks, which wait for B's attention blocks queued behind A's: r06 saw exactly this as an intermittent 0.5 s time-out with eight
    // ranks on one GPU.  A process that owns its device cannot starve itself (its own lower-index blocks are always dispatched first).
    const bool shared_dev = vh_tuning()->comm_ranks_per_device > 1 || (m->comm && vh_comm_ranks_per_device(m->comm) > 1);
    const bool fused_attn = fused_wanted(m) && !shared_dev;
    m->schedule_state = fused_attn ? 1 : 0;
    int* err = u.counters + 3;
    VhXchg xa{}, xm{};                           // attention / MoE exchange of the current layer
    bool have_xm = false;
    for (int l = 0; l < m->c.n_layers; ++l) {
        const vh_mixtral_layer& w = m->L[l];
        const VhExperts& ex = m->X[l];
        float* kc = m->kcache + (size_t)l * nkv * m->c.max_ctx * hd;
        float* vc = m->vcache + (size_t)l * nkv * m->c.max_ctx * hd;
        const bool prof = m->prof_stride > 0 && (l % m->prof_stride) == 0 && m->prof_used + 2 <= m->prof_ev.size();
        if (fuse && vh_comm_xchg_next(m->comm, H, 0, vhk_dec_gateup_blocks(ex.fmt, I, H), &xa, st) != VH_OK)
            return fail(VH_E_COMM, "fused exchange failed: %s", vh_comm_last_error());
        if (fused_attn) {
            VhDecAblk a{};
            a.x_in = u.xa; a.delta = l == 0 ? nullptr : u.dm; a.x_out = u.xb; a.norm_w = w.attn_norm; a.eps = eps;
            a.Wqkv = w.wqkv; a.nqkv = m->nqkv; a.H = H;
            a.kcache = kc; a.vcache = vc; a.pos = u.host_pos; a.table = u.table; a.rope_cos = m->rope_cos; a.rope_sin = m->rope_sin;
            a.part_o = m->part_o; a.part_ml = m->part_ml; a.cnt = m->attn_cnt; a.nq = nq; a.nkv = nkv; a.max_ctx = m->c.max_ctx;
            a.max_splits = m->max_splits; a.nsplit = (u.host_pos + 1 + 63) / 64; a.scale = scale;
            a.Wo = w.wo; a.out = u.da;
            a.gq = VhGranVec{m->g_qkv, m->next_tag(), err}; a.ga = VhGranVec{m->g_attn, m->next_tag(), err};
            if (have_xm) a.cx = xm;
            if (fuse) a.px = xa;
            VH_TRY(vhk_dec_ablk(st, a), "dec attention block");
        } else {
            VH_TRY(vhk_dec_qkv(st, u.xa, l == 0 ? nullptr : u.dm, u.xb, w.attn_norm, eps, w.wqkv, m->nqkv, H,
                               m->qkv, have_xm ? &xm : nullptr), "dec qkv");
            VH_TRY(vhk_dec_attn(st, m->qkv, kc, vc, u.counters, m->rope_cos, m->rope_sin, m->part_o, m->part_ml,
                                m->attn_cnt, m->attn_out, nq, nkv, m->c.max_ctx, m->max_splits, u.host_pos + 1,
                                scale, u.table), "dec attn");
            VH_TRY(vhk_dec_oproj(st, m->attn_out, w.wo, H, nq * hd, u.da, fuse ? &xa : nullptr), "dec oproj");
        }
        if (!fuse && m->allreduce(u.da, H, st) != 0) return fail(VH_E_COMM, "all-reduce failed");
        // the consumer of the MoE exchange is the next layer's attention block (or fused-QKV GEMV), or the LM head after the last layer
        const int xm_blocks = l + 1 < m->c.n_layers ? (fused_attn ? vhk_dec_ablk_qkv_blocks(m->nqkv, H) : vhk_dec_qkv_blocks(m->nqkv))
                                                     : m->lm_grid;
        if (prof) (void)hipEventRecord(m->prof_ev[m->prof_used], st);
        VH_TRY(vhk_dec_gateup(st, u.xb, u.da, u.xa, w.ffn_norm, eps, w.wrouter, m->E, ex, I, H, m->route, m->hbuf, 0, fuse ? &xa : nullptr), "dec gateup");
        if (prof) { (void)hipEventRecord(m->prof_ev[m->prof_used + 1], st); m->prof_used += 2; }
        if (fuse) {
            if (vh_comm_xchg_next(m->comm, H, 1, xm_blocks, &xm, st) != VH_OK) return fail(VH_E_COMM, "fused exchange failed: %s", vh_comm_last_error());
            have_xm = true;
        }
        VH_TRY(vhk_dec_down(st, m->hbuf, m->route, ex, H, I, u.dm, fuse ? &xm : nullptr), "dec down");
        if (!fuse && m->allreduce(u.dm, H, st) != 0) return fail(VH_E_COMM, "all-reduce failed");
    }
    const int rc = head_one(m, st, u, u.xa, u.dm, /*mode=*/1, /*set_pos=*/0, have_xm ? &xm : nullptr);
    if (rc != VH_OK) return rc;
    const hipError_t e = hipGetLastError();   // checked per step: the mirrors must not run ahead of a failed launch
    if (e != hipSuccess) return fail(VH_E_HIP, "decode: %s", hipGetErrorString(e));
    return VH_OK;
}

// The host mirrors of a decode step move here, for the step of one unit and for every member of a batched iteration alike: a step that
// was enqueued whole advances the position; one that was not poisons its unit and leaves host_pos at the last COMPLETE step (the device
// state of the partial step is discarded by unit 0's next prefill / reset; a slot is lost until it is freed).
static int settle_step(vh_mixtral::Unit& u, int rc) {
    if (rc == VH_OK) u.host_pos += 1;
    else u.poisoned = 1;
    return rc;
}
static int step_unit(vh_mixtral* m, vh_mixtral::Unit& u, hipStream_t st) { return settle_step(u, decode_one_step(m, u, st)); }

int vh_mixtral_decode(vh_mixtral_t* m, int n_steps, void* stream) {
    if (!m) return fail(VH_E_ARG, "null engine");
    vh_mixtral::Unit& u = m->units[0];
    if (u.poisoned) return fail(VH_E_ARG, "decode: a previous step failed; prefill or reset first");
    if (m->live_seqs() > 0) return fail(VH_E_ARG, "vh_mixtral_decode: sequences own pages of the KV pool (use vh_mixtral_seq_decode)");
    if (m->pages_in_use())
        return fail(VH_E_ARG, "%s: pages of the KV pool are held (vh_mixtral_seq_hold_prefix; serving: the prefix cache): release them "
                              "(vh_mixtral_pages_release / reset_prefix_cache) or reset", "vh_mixtral_decode");
    for (int step = 0; step < n_steps; ++step) {
        if (u.host_pos + 1 >= m->c.max_ctx) return fail(VH_E_SHAPE, "decode: KV cache full (%d)", m->c.max_ctx);
        const int rc = step_unit(m, u, S(stream));
        if (rc != VH_OK) return rc;
    }
    return VH_OK;
}

// ---- concurrent sequences (paged KV cache) ---------------------------------------------------------------------------
static int seq_ok(vh_mixtral* m, int s, const char* what) {
    if (!m) return fail(VH_E_ARG, "%s: null engine", what);
    if (s < 0 || s >= (int)m->seqs.size() || !m->seqs[s].live) return fail(VH_E_ARG, "%s: sequence %d is not allocated", what, s);
    return VH_OK;
}

int vh_mixtral_seq_alloc(vh_mixtral_t* m) {
    if (!m) return fail(VH_E_ARG, "null engine");
    for (int s = 0; s < (int)m->seqs.size(); ++s)
        if (!m->seqs[s].live) { m->seqs[s].live = true; m->slot(s).samp = VhSampleParams{}; m->slot(s).rules = vh_mixtral::Rules{}; return s; }
    return fail(VH_E_FULL, "vh_mixtral_seq_alloc: all %d sequence slots are in use", (int)m->seqs.size());
}

int vh_mixtral_seq_free(vh_mixtral_t* m, int s) {
    const int rc = seq_ok(m, s, "vh_mixtral_seq_free");
    if (rc != VH_OK) return rc;
    m->release(s);
    return VH_OK;
}

int vh_mixtral_seq_set_sampling(vh_mixtral_t* m, int s, const vh_sampling* smp) {
    const int rc0 = seq_ok(m, s, "vh_mixtral_seq_set_sampling");
    if (rc0 != VH_OK) return rc0;
    VhSampleParams p;
    const int rc = engine_sampling(m, smp, &p, "vh_mixtral_seq_set_sampling");
    if (rc != VH_OK) return rc;
    m->slot(s).samp = p;
    return VH_OK;
}

int vh_mixtral_seq_set_logit_rules(vh_mixtral_t* m, int s, const vh_logit_rules* r, const int* ids, int n_prompt, int n_output) {
    const int rc0 = seq_ok(m, s, "vh_mixtral_seq_set_logit_rules");
    if (rc0 != VH_OK) return rc0;
    return engine_rules(m, m->slot(s), r, ids, n_prompt, n_output, "vh_mixtral_seq_set_logit_rules");
}
// accessors: the engine-level ones read unit 0, the per-slot ones the slot's record.  seq_pos / seq_table answer for a LIVE slot only;
// the buffer getters answer for any slot index (a freed sequence's ids and counters can still be read)
static bool slot_ok(const vh_mixtral_t* m, int s) { return m && s >= 0 && s < (int)m->seqs.size(); }
static bool live_ok(const vh_mixtral_t* m, int s) { return slot_ok(m, s) && m->seqs[s].live; }
const float* vh_mixtral_logprobs_token(const vh_mixtral_t* m) { return m ? m->units[0].lp_tok : nullptr; }
const int* vh_mixtral_logprobs_top_ids(const vh_mixtral_t* m) { return m ? m->units[0].lp_top_id : nullptr; }
const float* vh_mixtral_logprobs_top(const vh_mixtral_t* m) { return m ? m->units[0].lp_top : nullptr; }
const float* vh_mixtral_seq_logprobs_token(const vh_mixtral_t* m, int s) { return slot_ok(m, s) ? m->slot(s).lp_tok : nullptr; }
const int* vh_mixtral_seq_logprobs_top_ids(const vh_mixtral_t* m, int s) { return slot_ok(m, s) ? m->slot(s).lp_top_id : nullptr; }
const float* vh_mixtral_seq_logprobs_top(const vh_mixtral_t* m, int s) { return slot_ok(m, s) ? m->slot(s).lp_top : nullptr; }
const uint32_t* vh_mixtral_seen(const vh_mixtral_t* m) { return m ? m->units[0].seen : nullptr; }
const uint32_t* vh_mixtral_seq_seen(const vh_mixtral_t* m, int s) { return slot_ok(m, s) ? m->slot(s).seen : nullptr; }

int vh_mixtral_pages_free(const vh_mixtral_t* m) { return m ? (int)m->free_pages.size() : 0; }
int vh_mixtral_seq_pos(const vh_mixtral_t* m, int s) { return live_ok(m, s) ? m->slot(s).host_pos : -1; }
const int* vh_mixtral_seq_tokens(const vh_mixtral_t* m, int s) { return slot_ok(m, s) ? m->slot(s).tokens : nullptr; }
const int* vh_mixtral_seq_counters(const vh_mixtral_t* m, int s) { return slot_ok(m, s) ? m->slot(s).counters : nullptr; }
int vh_mixtral_seq_table(const vh_mixtral_t* m, int s, int* pages_out, int cap) {
    if (!live_ok(m, s)) return -1;
    const vh_mixtral::Seq& q = m->seqs[s];
    for (int j = 0; j < q.npages && j < cap; ++j) pages_out[j] = q.pages[j];
    return q.npages;
}

// ---- shared pages (prefix caching): holds, release, adoption.  Host calls; each checks the WHOLE call before it changes anything.
int vh_mixtral_page_refs(const vh_mixtral_t* m, int page) {
    return m && page >= 0 && page < (int)m->page_refs.size() ? m->page_refs[page] : -1;
}

int vh_mixtral_seq_hold_prefix(vh_mixtral_t* m, int s, int n_pages, int* pages_out) {
    const char* what = "vh_mixtral_seq_hold_prefix";
    const int rc = seq_ok(m, s, what);
    if (rc != VH_OK) return rc;
    if (!pages_out) return fail(VH_E_ARG, "%s: null pointer", what);
    if (m->slot(s).poisoned) return fail(VH_E_ARG, "sequence %d: a previous step failed; free it", s);
    if (n_pages < 1 || 64L * n_pages > m->slot(s).host_pos)
        return fail(VH_E_ARG, "%s: %d pages are not all below position %d of sequence %d (only full pages can be held)", what, n_pages,
                    m->slot(s).host_pos, s);
    const vh_mixtral::Seq& q = m->seqs[s];
    for (int j = 0; j < n_pages; ++j) { m->page_refs[q.pages[j]] += 1; pages_out[j] = q.pages[j]; }
    return VH_OK;
}

int vh_mixtral_pages_release(vh_mixtral_t* m, const int* pages, int n) {
    const char* what = "vh_mixtral_pages_release";
    if (!m || (!pages && n > 0)) return fail(VH_E_ARG, "%s: null pointer", what);
    if (n < 0) return fail(VH_E_ARG, "%s: n = %d", what, n);
    std::vector<int> drop(m->page_refs.size(), 0);
    for (int i = 0; i < n; ++i) {
        const int pg = pages[i];
        if (pg < 0 || pg >= (int)drop.size()) return fail(VH_E_ARG, "%s: page %d outside [0,%d)", what, pg, (int)drop.size());
        if (++drop[pg] > m->page_refs[pg])
            return fail(VH_E_ARG, "%s: page %d is listed %d times and has %d references", what, pg, drop[pg], m->page_refs[pg]);
    }
    for (int i = n - 1; i >= 0; --i) m->unref_page(pages[i]);   // last listed first: as seq_free returns a table
    return VH_OK;
}

int vh_mixtral_seq_adopt(vh_mixtral_t* m, int s, const int* pages, int n, void* stream) {
    const char* what = "vh_mixtral_seq_adopt";
    const int rc = seq_ok(m, s, what);
    if (rc != VH_OK) return rc;
    if (!pages) return fail(VH_E_ARG, "%s: null pointer", what);
    vh_mixtral::Seq& q = m->seqs[s];
    vh_mixtral::Unit& u = m->slot(s);
    if (u.poisoned) return fail(VH_E_ARG, "sequence %d: a previous step failed; free it", s);
    if (u.host_pos != 0 || q.npages != 0)
        return fail(VH_E_ARG, "%s: sequence %d is at position %d with %d pages (only a new sequence adopts)", what, s, u.host_pos, q.npages);
    if (n < 1 || n > m->max_splits || 64L * n + 1 >= m->c.max_ctx)
        return fail(VH_E_ARG, "%s: %d pages outside [1,%d] or no room for a token behind them (pool %d tokens)", what, n, m->max_splits,
                    m->c.max_ctx);
    for (int i = 0; i < n; ++i) {
        const int pg = pages[i];
        if (pg < 0 || pg >= (int)m->page_refs.size() || m->page_refs[pg] < 1)
            return fail(VH_E_ARG, "%s: page %d is free or out of range", what, pg);
        for (int j = 0; j < i; ++j)
            if (pages[j] == pg) return fail(VH_E_ARG, "%s: page %d is listed twice", what, pg);
    }
    hipStream_t st = S(stream);
    for (int i = 0; i < n; ++i) q.pages[i] = pages[i];          // the upload reads the mirror (entries above npages are unused)
    if (hipMemcpyAsync(u.table, q.pages.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(u.counters), 64 * n, 1, st) != hipSuccess)
        return fail(VH_E_HIP, "%s: table / position upload failed", what);
    for (int i = 0; i < n; ++i) m->page_refs[pages[i]] += 1;
    q.npages = n;
    u.host_pos = 64 * n;
    return VH_OK;
}

int vh_mixtral_seq_prefill(vh_mixtral_t* m, int s, const float* embeds, int Sn, float* logits_out, void* stream) {
    const int rc0 = seq_ok(m, s, "vh_mixtral_seq_prefill");
    if (rc0 != VH_OK) return rc0;
    if (!embeds) return fail(VH_E_ARG, "vh_mixtral_seq_prefill: null pointer");
    hipStream_t st = S(stream);
    const int pos0 = m->slot(s).host_pos;       // appends to the sequence (0 for a new one): chunked prompts, later turns
    if (Sn < 1 || pos0 + Sn >= m->c.max_ctx) return fail(VH_E_SHAPE, "prefill of %d tokens at %d exceeds the pool", Sn, pos0);
    const int pr = m->ensure_pages(s, pos0 + Sn, st);
    if (pr == -1) return fail(VH_E_FULL, "KV pool exhausted: %d pages free, sequence %d needs %d more", (int)m->free_pages.size(),
                              s, (pos0 + Sn + 63) / 64 - m->seqs[s].npages);
    if (pr != 0) return fail(VH_E_HIP, "page table upload failed");
    const PfSeg one{1 + s, Sn, pos0};
    return prefill_impl(m, embeds, &one, 1, logits_out, nullptr, st);
}

int vh_mixtral_seq_prefill_batch(vh_mixtral_t* m, const int* seqs, const int* lens, int n, const float* embeds, float* logits_out,
                                 void* stream) {
    const char* what = "vh_mixtral_seq_prefill_batch";
    if (!m || !seqs || !lens || !embeds) return fail(VH_E_ARG, "%s: null pointer", what);
    if (n < 1 || n > (int)m->seqs.size()) return fail(VH_E_ARG, "%s: %d segments outside [1,%d]", what, n, (int)m->seqs.size());
    hipStream_t st = S(stream);
    // the whole call is checked before anything is enqueued or allocated
    long rows = 0, pages = 0;
    for (int i = 0; i < n; ++i) {
        const int rc = seq_ok(m, seqs[i], what);
        if (rc != VH_OK) return rc;
        const vh_mixtral::Seq& q = m->seqs[seqs[i]];
        const int pos = m->slot(seqs[i]).host_pos;
        if (m->slot(seqs[i]).poisoned) return fail(VH_E_ARG, "sequence %d: a previous step failed; free it", seqs[i]);
        for (int j = 0; j < i; ++j)
            if (seqs[j] == seqs[i]) return fail(VH_E_ARG, "%s: sequence %d is listed twice", what, seqs[i]);
        if (lens[i] < 1) return fail(VH_E_SHAPE, "%s: segment %d has %d rows", what, i, lens[i]);
        if (pos + (long)lens[i] >= m->c.max_ctx)
            return fail(VH_E_SHAPE, "prefill of %d tokens at %d exceeds the pool", lens[i], pos);
        rows += lens[i];
        const int need = (pos + lens[i] + 63) / 64;
        if (need > q.npages) pages += need - q.npages;
    }
    if (rows > m->c.max_prefill) return fail(VH_E_SHAPE, "%s: %ld rows exceed max_prefill %d", what, rows, m->c.max_prefill);
    if (pages > (long)m->free_pages.size())
        return fail(VH_E_FULL, "KV pool exhausted: %d pages free, the %d segments need %ld more", (int)m->free_pages.size(), n, pages);
    if (n == 1) return vh_mixtral_seq_prefill(m, seqs[0], embeds, lens[0], logits_out, stream);
    std::vector<PfSeg> sg(n);
    std::vector<int> had(n);
    for (int i = 0; i < n; ++i) had[i] = m->seqs[seqs[i]].npages;
    for (int i = 0; i < n; ++i) {
        sg[i] = PfSeg{1 + seqs[i], lens[i], m->slot(seqs[i]).host_pos};
        if (m->ensure_pages(seqs[i], sg[i].pos0 + lens[i], st) != 0) {
            for (int j = i; j >= 0; --j) {          // pages taken for this call go back, in the order they would be handed out again
                vh_mixtral::Seq& r = m->seqs[seqs[j]];
                while (r.npages > had[j]) m->unref_page(r.pages[--r.npages]);
            }
            return fail(VH_E_HIP, "page table upload failed");
        }
    }
    return prefill_impl(m, embeds, sg.data(), n, logits_out, nullptr, st);   // enqueued in part: exactly the listed sequences are lost
}

int vh_mixtral_seq_step(vh_mixtral_t* m, const int* pf_seqs, const int* pf_lens, int n_pf, const float* embeds, const int* dec_seqs,
                        int n_dec, float* logits_out, void* stream) {
    const char* what = "vh_mixtral_seq_step";
    if (!m || (n_pf > 0 && (!pf_seqs || !pf_lens || !embeds)) || (n_dec > 0 && !dec_seqs)) return fail(VH_E_ARG, "%s: null pointer", what);
    if (n_pf < 0 || n_dec < 0 || n_pf + n_dec < 1 || n_pf + (long)n_dec > (long)m->seqs.size())
        return fail(VH_E_ARG, "%s: %d prompt segments and %d decode members outside [1,%d] together", what, n_pf, n_dec, (int)m->seqs.size());
    if (n_dec == 0) return vh_mixtral_seq_prefill_batch(m, pf_seqs, pf_lens, n_pf, embeds, logits_out, stream);
    hipStream_t st = S(stream);
    // the whole call is checked before anything is enqueued or allocated
    const int n = n_pf + n_dec;
    long rows = 0, pages = 0;
    for (int i = 0; i < n; ++i) {
        const bool dec = i >= n_pf;
        const int s = dec ? dec_seqs[i - n_pf] : pf_seqs[i];
        const int rc = seq_ok(m, s, what);
        if (rc != VH_OK) return rc;
        const int pos = m->slot(s).host_pos, len = dec ? 1 : pf_lens[i];
        if (m->slot(s).poisoned) return fail(VH_E_ARG, "sequence %d: a previous step failed; free it", s);
        for (int j = 0; j < i; ++j)
            if ((j >= n_pf ? dec_seqs[j - n_pf] : pf_seqs[j]) == s) return fail(VH_E_ARG, "%s: sequence %d is listed twice", what, s);
        if (len < 1) return fail(VH_E_SHAPE, "%s: segment %d has %d rows", what, i, len);
        if (dec && pos < 1) return fail(VH_E_ARG, "sequence %d has no prompt yet", s);
        if (pos + (long)len >= m->c.max_ctx)
            return dec ? fail(VH_E_SHAPE, "sequence %d: context limit %d", s, m->c.max_ctx)
                       : fail(VH_E_SHAPE, "prefill of %d tokens at %d exceeds the pool", len, pos);
        rows += len;
        const int need = (pos + len + 63) / 64;
        if (need > m->seqs[s].npages) pages += need - m->seqs[s].npages;
    }
    if (rows > m->c.max_prefill) return fail(VH_E_SHAPE, "%s: %ld rows exceed max_prefill %d", what, rows, m->c.max_prefill);
    if (pages > (long)m->free_pages.size())
        return fail(VH_E_FULL, "KV pool exhausted: %d pages free, the %d members need %ld more", (int)m->free_pages.size(), n, pages);
    std::vector<PfSeg> sg(n);
    std::vector<int> ids(n), had(n);
    for (int i = 0; i < n; ++i) { ids[i] = i >= n_pf ? dec_seqs[i - n_pf] : pf_seqs[i]; had[i] = m->seqs[ids[i]].npages; }
    for (int i = 0; i < n; ++i) {
        sg[i] = PfSeg{1 + ids[i], i >= n_pf ? 1 : pf_lens[i], m->slot(ids[i]).host_pos, i >= n_pf ? 1 : 0};
        if (m->ensure_pages(ids[i], sg[i].pos0 + sg[i].len, st) != 0) {
            for (int j = i; j >= 0; --j) {          // pages taken for this call go back, in the order they would be handed out again
                vh_mixtral::Seq& r = m->seqs[ids[j]];
                while (r.npages > had[j]) m->unref_page(r.pages[--r.npages]);
            }
            return fail(VH_E_HIP, "page table upload failed");
        }
    }
    return prefill_impl(m, embeds, sg.data(), n, logits_out, nullptr, st);   // enqueued in part: exactly the listed sequences are lost
}

// One decode ITERATION of n concurrent sequences (n <= max_seqs, all distinct).  The attention side (fused QKV GEMV,
// split-KV attention, O projection) and the LM head run in groups of up to VH_BMAX sequences per launch (one pass over
// the shared weights per group).  The MoE of a layer runs
//   n >= batch_moe_min (default 3): ONCE for the whole iteration on the prefill's weight-streaming GEMM with S = n — rows
//       sorted by expert, every TOUCHED expert streamed exactly once at ~5 TB/s however many sequences picked it
//       (k_gemm_ps cfg 0, <= 64 rows per tile — with its few-row rules: vh_gemm_ps_inl.h K-split estimator, vh_gemm_ps.hip cache hint;
//       "continuous batching");
//   otherwise per sequence with the batch-1 GEMV kernels.
// Sequence state is addressed in place (the slots' records); under the streaming MoE the delta of a sequence is a row of the shared
// `ptmp` buffer.
static int decode_iteration(vh_mixtral* m, hipStream_t st, const int* ids, int n) {
    const int H = m->H, I = m->I, E = m->E, nq = m->nq, nkv = m->nkv, hd = m->hd;
    const float scale = 1.0f / sqrtf((float)hd);
    const float eps = m->c.rms_eps;
    const bool tp = m->c.tp_world > 1 || vh_tuning()->force_allreduce;
    std::vector<vh_mixtral::Unit*> us(n);
    std::vector<const float*> xa(n);
    std::vector<float*> dm(n);     // MoE delta of sequence b: its own, or its row of ptmp
    for (int b = 0; b < n; ++b) { us[b] = &m->slot(ids[b]); xa[b] = us[b]->xa; dm[b] = us[b]->dm; }
    const int moe_min = vh_tuning()->batch_moe_min;
    const bool stream_moe = moe_min > 0 && n >= moe_min && n <= m->c.max_prefill && H <= 4096 && (H % 64) == 0 && (I % 64) == 0;
    if (stream_moe) {
        // the slot list of the iteration lives on the device for k_gather_rows; it is re-uploaded only when the running
        // set changed (a pageable-memory upload waits for the stream: doing it every iteration would stop the host from
        // enqueueing ahead of the GPU).  The source is a member whose storage never moves (reserved at creation).
        if ((int)m->batch_ids_host.size() != n || memcmp(m->batch_ids_host.data(), ids, (size_t)n * sizeof(int)) != 0) {
            m->batch_ids_host.assign(ids, ids + n);
            if (hipMemcpyAsync(m->seq_batch, m->batch_ids_host.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess)
                return fail(VH_E_HIP, "batch id upload failed");
        }
        for (int b = 0; b < n; ++b) dm[b] = m->ptmp + (size_t)b * H;       // MoE delta rows of this iteration
    }
    for (int l = 0; l < m->c.n_layers; ++l) {
        const vh_mixtral_layer& w = m->L[l];
        const VhExperts& ex = m->X[l];
        float* kc = m->kcache + (size_t)l * nkv * m->c.max_ctx * hd;
        float* vc = m->vcache + (size_t)l * nkv * m->c.max_ctx * hd;
        for (int g0 = 0; g0 < n; g0 += VH_BMAX) {
            const int gn = n - g0 < VH_BMAX ? n - g0 : VH_BMAX;
            VhDecBatchVec q{};
            VhDecBatchAttn at{};
            VhDecBatchVec o{};
            q.n = gn; o.n = gn;
            for (int b = 0; b < gn; ++b) {
                const int sb = g0 + b;
                const vh_mixtral::Unit& u = *us[sb];
                q.x_in[b] = u.xa; q.delta[b] = l == 0 ? nullptr : dm[sb]; q.x_out[b] = u.xb; q.out[b] = m->l_qkv[b];
                at.qkv[b] = m->l_qkv[b]; at.pos[b] = u.host_pos;
                at.table[b] = u.table;
                at.part_o[b] = m->l_part_o[b]; at.part_ml[b] = m->l_part_ml[b]; at.cnt[b] = m->l_attn_cnt[b];
                at.attn_out[b] = m->l_attn_out[b];
                o.x_in[b] = m->l_attn_out[b]; o.out[b] = u.da;
            }
            VH_TRY(vhk_decb_gemv(st, q, w.attn_norm, eps, w.wqkv, m->nqkv, H, 1), "batched qkv");
            VH_TRY(vhk_decb_attn(st, at, gn, kc, vc, m->rope_cos, m->rope_sin, nq, nkv, m->c.max_ctx, m->max_splits, scale), "batched attn");
            VH_TRY(vhk_decb_gemv(st, o, nullptr, 0.f, w.wo, H, nq * hd, 0), "batched oproj");
        }
        for (int b = 0; b < n; ++b)
            if (m->allreduce(us[b]->da, H, st) != 0) return fail(VH_E_COMM, "all-reduce failed");
        if (stream_moe) {
            // x = xb + delta_attn for every sequence -> rows of px (and each sequence's xa, as the GEMV path's x_out)
            VH_TRY(vhk_gather_rows(st, m->seq_x, m->seq_batch, n, H, m->px), "gather");
            VH_TRY(vhk_rmsnorm_route(st, m->px, nullptr, m->pxn_hi, m->pxn_lo, w.ffn_norm, n, H, eps, w.wrouter, E, m->pids,
                                     m->pwts), "rmsnorm + route");
            MoeGemms moe;
            int rc = moe_gemms(m, st, w, n, &moe);
            if (rc != VH_OK) return rc;
            VH_TRY(moe_gate_up(st, moe), "gate/up gemm");
            if ((rc = moe_down(m, st, moe, n, 0, H, m->ptmp)) != VH_OK) return rc;
            if (tp && m->allreduce(m->ptmp, (long)n * H, st) != 0) return fail(VH_E_COMM, "all-reduce failed");
        } else {
            for (int b = 0; b < n; ++b) {
                const vh_mixtral::Unit& u = *us[b];
                const int lane = b % VH_BMAX;   // the scratch lane the sequence had in its attention group
                VH_TRY(vhk_dec_gateup(st, u.xb, u.da, u.xa, w.ffn_norm, eps, w.wrouter, E, ex, I, H, m->l_route[lane], m->l_hbuf[lane], 0), "dec gateup");
                VH_TRY(vhk_dec_down(st, m->l_hbuf[lane], m->l_route[lane], ex, H, I, dm[b]), "dec down");
            }
            for (int b = 0; b < n; ++b)
                if (m->allreduce(dm[b], H, st) != 0) return fail(VH_E_COMM, "all-reduce failed");
        }
    }
    HeadArgs ha;   // a decode step: one score row per member, no fused exchange, loop-back does not count as sharded
    ha.sharded = m->head_sharded(/*loopback_counts=*/false);
    const int rc = head(m, st, us.data(), n, xa.data(), dm.data(), ha);
    if (rc != VH_OK) return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VH_E_HIP, "batched decode: %s", hipGetErrorString(e));
    return VH_OK;
}

int vh_mixtral_seq_decode(vh_mixtral_t* m, const int* ids, int n, void* stream) {
    if (!m || (!ids && n > 0)) return fail(VH_E_ARG, "vh_mixtral_seq_decode: null pointer");
    hipStream_t st = S(stream);
    for (int i = 0; i < n; ++i) {               // validate the whole batch before anything is enqueued
        const int rc = seq_ok(m, ids[i], "vh_mixtral_seq_decode");
        if (rc != VH_OK) return rc;
        const vh_mixtral::Unit& q = m->slot(ids[i]);
        if (q.poisoned) return fail(VH_E_ARG, "sequence %d: a previous step failed; free it", ids[i]);
        if (q.host_pos < 1) return fail(VH_E_ARG, "sequence %d has no prompt yet", ids[i]);
        if (q.host_pos + 1 >= m->c.max_ctx) return fail(VH_E_SHAPE, "sequence %d: context limit %d", ids[i], m->c.max_ctx);
    }
    // distinct sequences advance together through the batched iteration (a sequence listed twice in one call advances
    // twice, one step after the other, as before)
    if (n >= 2 && vh_tuning()->batch_decode != 0 && m->H <= 4096 && m->nq * m->hd <= 4096) {
        bool distinct = true;
        for (int i = 0; i < n && distinct; ++i)
            for (int j = 0; j < i; ++j) if (ids[i] == ids[j]) { distinct = false; break; }
        if (distinct) {
            for (int i = 0; i < n; ++i) {
                const int pr = m->ensure_pages(ids[i], m->slot(ids[i]).host_pos + 1, st);
                if (pr == -1) return fail(VH_E_FULL, "KV pool exhausted at sequence %d (nothing of the batch advanced)", ids[i]);
                if (pr != 0) return fail(VH_E_HIP, "page table upload failed");
            }
            const int rc = decode_iteration(m, st, ids, n);
            for (int i = 0; i < n; ++i) settle_step(m->slot(ids[i]), rc);   // a failed iteration poisons exactly the listed slots
            return rc;
        }
    }
    for (int i = 0; i < n; ++i) {
        const int s = ids[i];
        const int pr = m->ensure_pages(s, m->slot(s).host_pos + 1, st);   // the step writes K/V of position host_pos
        if (pr == -1) return fail(VH_E_FULL, "KV pool exhausted at sequence %d (%d of the batch advanced)", s, i);
        if (pr != 0) return fail(VH_E_HIP, "page table upload failed");
        const int rc = step_unit(m, m->slot(s), st);
        if (rc != VH_OK) return rc;
    }
    return VH_OK;
}

}  // extern "C"
