/* vita_hip.h — C ABI of libvita_hip.so, the MI355X (gfx950) hot path of VITA inference.
 *
 * The reference (VITA-MLLM/VITA @ 2024-10-22) is 100 % Python and has no FFI of its own:
 * its drop-in boundary is the `vita.model` Python API (vita/model/builder.py:14-24,306;
 * vita/model/language_model/vita_mixtral.py:249-415; vita/model/multimodal_encoder/builder.py:12,44;
 * vita/model/multimodal_projector/builder.py:154).  This header is the boundary we add
 * beneath it: the entry points a maintainer binds with ctypes from those Python classes
 * (see INTEGRATION.md).  Each function names the reference computation it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless marked host;
 *   - `stream` is a hipStream_t passed as void*; all work is asynchronous on it;
 *   - activations are fp32, large weights bf16 (uint16 storage), small vectors fp32;
 *   - return 0 on success, VH_E_* (<0) on error; vh_last_error() describes the last one;
 *   - no entry point allocates device memory; engines take a caller-provided workspace
 *     whose size comes from the matching *_workspace_bytes().
 */
#ifndef VITA_HIP_H
#define VITA_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VH_OK 0
#define VH_E_SHAPE (-1)
#define VH_E_ARG (-2)
#define VH_E_HIP (-3)
#define VH_E_COMM (-4)
#define VH_E_FULL (-5)   /* a pool is exhausted (sequence slots, KV pages): retry after freeing */

#define VH_ACT_NONE 0
#define VH_ACT_GELU 1 /* erf GELU (nn.GELU default) */
#define VH_ACT_RELU 2
#define VH_ACT_SILU 3

int vh_version(void);
const char* vh_last_error(void);
/* Kernel-variant knobs (22 keys: "batch_moe_min", "batch_decode", "attn_impl", "attn_fa", "attn_rows", "attn_ksplit",
 * "prefill_attn_gemm", "prefill_fuse_rows", "ps_cfg", "ps_nt", "tp_overlap", "moe_ksplit", "force_allreduce", "tp_fuse",
 * "comm_allow_coarse", "comm_ranks_per_device", "dec_fused", "dec_gateup_grid", "attn_img", "attn_xcd", "ps_xcd", "step_attn"; vita_amd/csrc/vh_kernels.h: VhTuning says what each selects); the defaults are the
 * measured-best variants, ids are identical across variants.  Unknown keys (e.g. of variants removed in r04) return VH_E_ARG. */
int vh_tune(const char* key, int value);

/* ---- generic operators --------------------------------------------------------------
 * vh_gemm: C = epilogue(A W^T).  Replaces every nn.Linear / conv-as-GEMM on the path:
 * InternViT qkv/proj/fc1/fc2 (internvit/modeling_intern_vit.py:144,175,213-217), the
 * mlp2x_gelu projector (multimodal_projector/builder.py:164-168), Whale linears and convs
 * (whale/module/component/subsampling.py:28-43, module/layer/attention.py:145-147,370-419,
 * adapter.py:93-136) and the Mixtral prefill projections + expert GEMMs (HF
 * modeling_mixtral.py MixtralAttention / MixtralExperts).
 *   A fp32 [*, lda]; logical row m reads source row a_rowidx[m] (or m) + segrow[k/seglen],
 *   column k%seglen; rows outside [0,a_rows) read as zero.  K = nseg*seglen, K%64==0.
 *   W bf16 [N][ldw]; W_up != NULL selects the gated form silu(A W^T) * (A W_up^T).
 *   group_off != NULL: grouped GEMM over `ngroups` row ranges, W advancing w_group_stride.
 *   epilogue: (+bias[n]) -> act -> (*scale[n]) -> (+resid[orow,n]) -> C[orow,n],
 *   orow = c_rowidx[m] or m.                                                            */
typedef struct {
    const float* A; long lda; int a_rows; const int* a_rowidx;
    int nseg; int seglen; int segrow[16];
    const uint16_t* W; const uint16_t* W_up; long ldw; long w_group_stride;
    const int* group_off; int ngroups;
    float* C; long ldc; const int* c_rowidx;
    const float* bias; const float* scale; const float* resid; long ldr;
    int M, N, K, act;
    float* ws; size_t ws_bytes;   /* optional scratch: lets small launches split K over more blocks (partial sums, then one
                                     reducing kernel that applies the epilogue); results differ from the unsplit launch
                                     only by fp32 summation order */
    int ksplit;                   /* 0 = decided by the library when ws != NULL, 1 = never split, n = n-way */
} vh_gemm_args;
int vh_gemm(const vh_gemm_args* args, void* stream);
/* vh_gemm_ln: vh_gemm followed by the LayerNorm that consumes its output, in one call:
 *   C = epilogue(A W^T)  and  ln_out[m, :] = LayerNorm(C[m, :]; ln_eps) * ln_w + ln_b      (ln_b nullable)
 * i.e. the encoders' `x = x + ls * proj(attn); h = norm2(x)` (InternVisionEncoderLayer.forward, modeling_intern_vit.py:245-253)
 * and Whale's `x = residual + feed_forward(x); x = norm(x)` steps.  When the library splits K (small launches) the
 * reducer holds whole rows and applies the norm itself; otherwise a norm launch follows.  Plain GEMMs only (no gate,
 * groups or output row map); N % 4 == 0. */
int vh_gemm_ln(const vh_gemm_args* args, const float* ln_w, const float* ln_b, float ln_eps, float* ln_out, long ld_ln,
               void* stream);

/* vh_gemm_ps: the same contraction as a WEIGHT STREAM for skinny M (Mixtral prefill, MoE grouped GEMMs: HF
 * MixtralExperts, modeling_mixtral.py:57-93) on activations already split into bf16 hi/lo planes (x = hi + lo
 * to 2^-17; vh_split_planes makes them, vh_gemm_ps can also emit them).  One m-tile covers all rows of a group
 * (up to 160 / 192; larger groups are cut into balanced m-tiles) so each weight byte is read once; K % 64 == 0,
 * lda % 8 == 0.  ksplit > 1 (plain fp32 output only): K is cut into ksplit ranges whose partial sums are
 * written to C + ks * c_split_stride (the caller adds the slabs).  `wide` is ignored (kept for ABI stability). */
typedef struct {
    const uint16_t* A_hi; const uint16_t* A_lo; long lda; const int* a_rowidx;
    const uint16_t* W; const uint16_t* W_up; long ldw; long w_group_stride;
    const int* group_off; int ngroups;
    float* C; long ldc; uint16_t* C_hi; uint16_t* C_lo; long ldc_split; const int* c_rowidx;
    const float* bias; const float* scale; const float* resid; long ldr;
    int M, N, K, act, wide;
    int ksplit; long c_split_stride;
    int* nslab_out;       /* ksplit < 0: the kernel picks the split (1 .. -ksplit) from the group sizes and stores it here (device int) */
} vh_gemm_ps_args;
int vh_gemm_ps(const vh_gemm_ps_args* args, void* stream);
int vh_split_planes(const float* x, long ldx, uint16_t* hi, uint16_t* lo, long ldo, int rows, int cols, void* stream);
/* vh_gemm_ps on int8 weights: args->W / W_up must be null; W (and W_up: GLU) int8 with args->ldw /
 * w_group_stride counted in int8 elements; column n of group e is scaled by s[e * s_group_stride + n] (s_up for the up half).
 * Always the 12-wave specialised kernel (vh_tune "ps_cfg" is ignored; "ps_xcd" and "ps_nt" apply).  Every int8 value is a legal
 * weight: -128, which vh_quant_rows_i8 never emits, is converted like the others and contributes exactly -128 s.  The weight
 * scale is applied to the K sum (each slab's under a K split) BEFORE bias, act, scale and resid.  Refused with VH_E_SHAPE, before
 * anything is launched or written: K % 64 != 0, ksplit > K / 64 or < -8, a K split (ksplit > 1 or < 0) with W_up, bias, scale,
 * resid, act or C_hi, ksplit < 0 without nslab_out, group_off with ngroups > 8, ldw * N >= 2^32. */
int vh_gemm_ps_i8(const vh_gemm_ps_args* args, const int8_t* W, const float* s, const int8_t* W_up, const float* s_up,
                  long s_group_stride, void* stream);
/* vh_gemm_ps on MXFP4 weights: args->W / W_up must be null; W (and W_up: GLU) are e2m1 codes, two per byte (element k
 * of a row in byte k >> 1, low nibble for even k), S (and S_up) one E8M0 scale byte per 32 consecutive elements of a row; the
 * weight is e2m1(code) * 2^(byte - 127), code 8 (-0) reads as 0.  args->ldw / w_group_stride count WEIGHTS: a code row is ldw / 2
 * bytes, a scale row ldw / 32 bytes, a group w_group_stride / 2 and w_group_stride / 32 bytes.  The conversion to bf16 is exact, so
 * the result is vh_gemm_ps's on the dequantised weights.  The contract covers scale bytes 2 to 252, which is what the quantiser
 * emits plus the range in which every w' is a normal bf16 number; other bytes are outside it (the kernel builds the scale as
 * byte << 23: byte 0 reads as 0.0 and 255 as Inf, byte 1 with code 1 is the bf16 denormal 2^-127, byte 253 with codes 6 and 7 and
 * byte 254 from code 4 upward exceed the bf16 range).  Always the 12-wave specialised kernel.  Refused with VH_E_SHAPE, before
 * anything is launched or written: ldw % 64 != 0, w_group_stride % 64 != 0, ldw < K, and what vh_gemm_ps_i8 refuses.  M == 0 is
 * accepted and writes nothing. */
int vh_gemm_ps_mxfp4(const vh_gemm_ps_args* args, const uint8_t* W, const uint8_t* S, const uint8_t* W_up, const uint8_t* S_up,
                     void* stream);

/* vh_attention: softmax(scale * Q K^T [+ (Q+v) P^T]) V with causal / pad / chunk masks.
 * Replaces InternAttention._naive_attn (modeling_intern_vit.py:158-177), Whale
 * MultiHeadedAttention.forward score/softmax/PV (attention.py:380-416) and HF
 * eager_attention_forward for the Mixtral prefill.  head_dim 64 or 128.
 * klens (nullable, device int[B]): batch b masks keys >= klens[b] — the per-utterance pad mask of a padded batch (Whale
 * `~make_pad_mask(xs_lens)`, whale/module/encoder/encoder.py:140-147; the serving plugin's one tower pass over padded clips,
 * web_demo/vllm_tools/vllm_file/mixtral.py:1043-1052); klen then carries max_b klens[b] (the launcher sizes the key split from it).
 * Honoured by the fp32 direct kernel (every rel-pos call; plain calls under vh_tune("attn_impl", 2) or a chunk mask); causal or
 * paged calls and the bf16 x 3 / flash kernels refuse it with VH_E_ARG.  klens == NULL: exactly the scalar-klen call. */
typedef struct {
    const float* Q; long ldq; long hsq;
    const float* K; long ldk; long hsk;
    const float* V; long ldv; long hsv;
    const float* P; long ldp; long hsp;
    const float* bias_u; const float* bias_v;
    float* O; long ldo;
    long bsq, bsk, bso;
    int B, Hq, Hkv, Sq, Sk, d;
    int causal, q_off, klen, chunk, left;
    float scale;
    const int* klens;
} vh_attn_args;
int vh_attention(const vh_attn_args* args, void* stream);

/* vh_encoder_layer: ONE pre-norm transformer block of the two encoders, all launches from a single call (the host loop of
 * 24 layers x 8 operator calls was slower than the GPU at one tile / one clip):
 *   qkv = h_in W_qkv^T + b;  a = attention(qkv);  x += ls1 * (a W_proj^T + b);  h = LN(x; n2);
 *   x += ls2 * (act(h W_fc1^T + b) W_fc2^T + b);  h_out = LN(x; next)                     (ls1 / ls2 / next nullable)
 * = InternVisionEncoderLayer.forward (internvit/modeling_intern_vit.py:245-253: layer scale, GELU) and Whale's
 * TransformerEncoderLayer.forward (whale/module/encoder/transformer.py, rel-pos attention whale/module/layer/attention.py:358-419:
 * P = linear_pos(pos_emb), pos_bias_u / pos_bias_v, pad / chunk mask; ReLU).  h_in is LN(x; this layer's norm1): from
 * vh_layernorm for the first layer, from the previous call's h_out afterwards.  Attention runs inside each of the B
 * sequences of M / B rows; keys >= klen are masked (klen < 0: none); klens (nullable, device int[B]) masks keys >= klens[b] in
 * sequence b instead (vh_attn_args.klens; klen then holds their maximum).  Rel-pos attention takes any B: P is indexed by the
 * position inside a sequence.  Scratch (caller-owned): qkv [M, 3C], attn [M, C], hmid [M, C], mid [M, F], ws (split-K slabs,
 * >= 32 M max(C, F) bytes recommended; 0 disables the split).
 * planes = 1 (r04; no rel-pos, ws >= 4 M C bytes): the rows that only feed the next Linear travel as the bf16 hi/lo planes vh_gemm_ps consumes — h_in / h_out,
 * attn and hmid then hold two planes each, hi [M][C] followed by lo [M][C] (mid: [M][F] twice), in the same M C 4 (M F 4) bytes — and the four Linears run on the
 * weight-streaming GEMM with one-round tilings (qkv / fc1 one pass; proj / fc2 K-split into ws, summed by the reducer that also applies bias, layer scale,
 * residual and the next LayerNorm).  Same arithmetic as planes = 0 (the general GEMM splits its fp32 operand into the same planes per block). */
typedef struct {
    float* x; const float* h_in; float* h_out;
    int M, C, F, heads, B;
    const uint16_t* qkv_w; const float* qkv_b;
    const uint16_t* proj_w; const float* proj_b; const float* ls1;
    const float* n2_w; const float* n2_b;
    const uint16_t* fc1_w; const float* fc1_b;
    const uint16_t* fc2_w; const float* fc2_b; const float* ls2;
    const float* next_w; const float* next_b;
    int act; float eps;
    const float* P; long ldp; const float* bias_u; const float* bias_v; int klen, chunk, left;
    float* qkv; float* attn; float* hmid; float* mid; float* ws; size_t ws_bytes;
    int planes;
    const int* klens;
} vh_encoder_layer_args;
int vh_encoder_layer(const vh_encoder_layer_args* args, void* stream);

/* nn.LayerNorm over the last dim (+ optional act, then * post_scale). */
int vh_layernorm(const float* x, long ldx, float* y, long ldy, const float* w, const float* b, int rows, int cols,
                 float eps, int act, float post_scale, void* stream);
/* MixtralRMSNorm (HF modeling_mixtral.py:134-148). */
int vh_rmsnorm(const float* x, float* y, const float* w, int rows, int cols, float eps, void* stream);
int vh_add(float* x, const float* y, long n, void* stream);
int vh_cast_bf16_f32(const uint16_t* in, float* out, long n, void* stream);
/* Content digests of embedded prompt rows, the keys of the serving layer's prefix cache (vLLM: enable_prefix_caching; its block
 * hashes are over token ids, which do not identify spliced image / audio rows, so here the rows themselves are hashed).
 * For every COMPLETE block b of 64 rows of x (fp32 [rows][cols], row stride ldx) one 128-bit digest out[b][0..4) over the raw 32-bit
 * patterns (-0.0 and 0.0 differ, NaN payloads count); a trailing partial block gets nothing, rows < 64 is VH_OK and writes nothing.
 * With word i = r * cols + c the pattern of x[64 b + r][c] (r < 64), all arithmetic modulo 2^32:
 *     fmix32(h):  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16      (MurmurHash3's finaliser)
 *     out[b][j] = fmix32( sum_i fmix32( word_i ^ fmix32(4 i + j + 0x9E3779B9) )  +  (j + 1) * 0x9E3779B9 ),   j = 0..3
 * - a function of the block's words and their positions inside the block only (not of b, ldx or the address); every reduction step
 * is a wrapping add, so the result does not depend on the grid or on the order of the partial sums.  A block is spread over 32
 * workgroups which add their partial sums into out (zeroed by this call) with vector integer atomics; a second tiny launch applies
 * the outer fmix32.  cols <= 2^23.  NOT cryptographic: whoever chooses the rows can construct collisions. */
int vh_hash_row_blocks(const float* x, long ldx, int rows, int cols, uint32_t* out /* device [rows / 64][4] */, void* stream);
/* Synthetic bf16 weights from a counter-based generator whose values are exact in bf16 (integers in [-126, 126] x 2^-11,
 * sigma 0.018): element (r, c) of the [rows, cols] view is sample idx0 + r * ld_src + c of stream `seed`, so shards of a
 * logical tensor hold the full tensor's values.  The host twin is oracle/hashfill.c — identical weights on both sides
 * at any size (no checkpoint exists offline: SURVEY 8(d)). */
int vh_fill_hash_bf16(uint16_t* dst, long rows, long cols, long ld_dst, long ld_src, long idx0, uint64_t seed, void* stream);

/* InternVisionEmbeddings + the first block's norm1 in ONE call (modeling_intern_vit.py:68-122, :243): patchify -> patch Linear
 * (+ bias) -> [cls | patches] + position table -> LayerNorm (-> bf16 hi / lo planes for vh_encoder_layer's planes mode).  Five
 * operator calls from Python left 177 us of host gaps in front of the first block of every tower pass (r04 trace); the pieces
 * stay available one by one below.  pos: the table ALREADY at this tile grid (the bicubic interpolation of the checkpoint's
 * table depends on the geometry only; the host does it once at load).  Scratch and outputs are caller-owned. */
typedef struct {
    const float* pix; int n, img, patch, kpad;            /* [n][3][img][img] fp32; kpad = padded 3 * patch^2 (multiple of 64) */
    const uint16_t* patch_w; const float* patch_b;         /* bf16 [C][kpad], fp32 [C] */
    const uint16_t* cls; const uint16_t* pos;              /* bf16 [C], bf16 [ntok][C] */
    const float* ln_w; const float* ln_b; float eps;
    int ntok, C;
    float* patches; float* pe;                             /* scratch: [n (img/patch)^2][kpad], [n (img/patch)^2][C] */
    float* x;                                              /* out: residual stream [n ntok][C] */
    float* h;                                              /* out: LayerNorm(x) fp32 [n ntok][C] */
    void* h_planes;                                        /* nullable out: the same rows as bf16 hi [n ntok][C] then lo [n ntok][C] */
    float* ws; size_t ws_bytes;                            /* nullable split-K scratch of the patch Linear */
} vh_vit_embed_args;
int vh_vit_embed(const vh_vit_embed_args* args, void* stream);

/* InternViT front/back (modeling_intern_vit.py:68-122; internvit_encoder.py:35-79). */
int vh_vit_patchify(const float* pix, float* out, int n, int img, int patch, int kpad, void* stream);
int vh_vit_assemble(const float* patches, const uint16_t* cls, const uint16_t* pos, float* x, int n, int ntok,
                    int hid, void* stream);
int vh_vit_pixel_shuffle(const float* x, float* out, int n, int grid, int hid, float mul, void* stream);

/* Whale GlobalCMVN + first Conv2d + ReLU, channels-last (cmvn.py:29-32; subsampling.py:28-31). */
int vh_audio_conv1(const float* feats, const float* mean, const float* istd, const uint16_t* w, const float* b,
                   float* out, int T, int F, int C, void* stream);
/* The same for B clips padded to a common length T in ONE launch: feats [B][T][F] -> out [B][T1][F1][C], clip after clip — the
 * front of the serving plugin's single tower pass over a padded batch (vllm_file/mixtral.py:861-886, 1043-1052; per clip the
 * arithmetic of vh_audio_conv1, bit for bit). */
int vh_audio_conv1_batch(const float* feats, const float* mean, const float* istd, const uint16_t* w, const float* b,
                         float* out, int B, int T, int F, int C, void* stream);
/* Tail of the padded batch: `xs = xs.masked_fill_(~mask_pad, 0)` in front of the adapter (whale/init_model.py:121-127, the
 * CNNSubsampling adapter then pads k - 1 zero frames on the right, adapter.py:93-136).  x [B][S][cols] (row stride ldx) ->
 * y [B][S + gap][cols] (row stride ldy): row s < klens[b] of clip b is copied, rows [klens[b], S + gap) are zeros, so that a
 * strided window over y that starts inside clip b never reads a neighbour's rows.  klens: device int[B]; cols % 4 == 0,
 * 16-byte aligned rows; x and y must not overlap. */
int vh_audio_mask_rows(const float* x, long ldx, float* y, long ldy, const int* klens, int B, int S, int gap, int cols,
                       void* stream);

/* embed_tokens gather + image/audio splice (vita_arch.py:237-321); kind 0 text,1 image,2 audio. */
int vh_embed_splice(const int* src_kind, const int* src_idx, const uint16_t* embed, const float* img_feats,
                    const float* aud_feats, float* out, int S, int H, void* stream);

/* ---- Mixtral engine: prefill + greedy decode (HF MixtralModel/GenerationMixin as driven by
 * vita_mixtral.py:101-215,291-382 and video_audio_demo.py:257-270) ---------------------- */
typedef struct {
    int hidden, n_layers, n_q_heads, n_kv_heads, head_dim, inter, n_experts, top_k, vocab;
    float rms_eps;
    int max_ctx;          /* KV-cache capacity in tokens */
    int max_prefill;      /* largest S accepted by vh_mixtral_prefill */
    int max_new;          /* capacity of the generated-token buffer */
    int tp_rank, tp_world;/* n_q_heads / n_kv_heads / inter above are THIS RANK's slices */
    int nsplit;           /* decode split-KV factor, 0 = auto */
    int logit_rows;       /* >1: keep the fp32 logits of the first logit_rows generated tokens */
    int vocab_lo, vocab_n;/* vocab-sharded LM head (ParallelLMHead, vllm_file/mixtral.py:939-951): `lm_head` holds rows
                             [vocab_lo, vocab_lo + vocab_n) of the table; the ranks exchange (max, index) candidates
                             through the all-reduce hook.  vocab_n == 0: the whole table on every rank. */
    int max_seqs;         /* > 0: slots for concurrent sequences over the paged KV cache (vh_mixtral_seq_*); max_ctx is then
                             the POOL size in tokens (a multiple of 64) shared by all sequences */
    int penalty_tables;   /* != 0: a token table uint32[vocab] for the engine and for every sequence slot (vh_logit_rules penalties) */
    int max_logprobs;     /* 1 .. 20: log-probability buffers for the engine and every slot ([max_new], [max_new][max_logprobs] x 2);
                             both 0: the workspace is what it was, the vh_logit_rules setters answer VH_E_ARG */
} vh_mixtral_cfg;

typedef struct {
    const float* attn_norm;    /* [hidden] fp32 */
    const uint16_t* wqkv;      /* [(nq+2nkv)*head_dim][hidden]  q rows, then k rows, then v rows */
    const uint16_t* wo;        /* [hidden][nq*head_dim] */
    const float* ffn_norm;     /* [hidden] */
    const uint16_t* wrouter;   /* [n_experts][hidden]   block_sparse_moe.gate */
    const uint16_t* w1;        /* [n_experts][inter][hidden]  gate proj (experts.N.w1) */
    const uint16_t* w3;        /* [n_experts][inter][hidden]  up proj   (experts.N.w3) */
    const uint16_t* w2;        /* [n_experts][hidden][inter]  down proj (experts.N.w2) */
} vh_mixtral_layer;

typedef struct vh_mixtral vh_mixtral_t;

size_t vh_mixtral_workspace_bytes(const vh_mixtral_cfg* cfg);
/* `layers` is a host array of cfg->n_layers entries (copied); a null w1 / w3 / w2 in layers[l] is refused (VH_E_ARG). rope tables:
 * fp32 [max_ctx][head_dim/2]. */
vh_mixtral_t* vh_mixtral_create(const vh_mixtral_cfg* cfg, const vh_mixtral_layer* layers, const uint16_t* embed,
                                const float* final_norm, const uint16_t* lm_head, const float* rope_cos,
                                const float* rope_sin, void* workspace, size_t workspace_bytes);
/* int8 experts (vLLM's quantization="experts_int8", the reference's load_8bit): the expert weights of every layer
 * as int8 with one fp32 scale per output row, s[r] = max_k |w[r,k]| / 127, q = clamp(rint(w / s), -127, 127) (vh_quant_rows_i8);
 * the engine computes with w' = q s.  w2's scales are over the FULL row of `inter` columns even when a tensor-parallel rank
 * stores only its column slice of q, so that every TP degree computes the same w'.  Activations stay fp32. */
typedef struct {
    const int8_t* w1; const float* s1;   /* [n_experts][inter][hidden] int8, [n_experts][inter] fp32 */
    const int8_t* w3; const float* s3;   /* [n_experts][inter][hidden] int8, [n_experts][inter] fp32 */
    const int8_t* w2; const float* s2;   /* [n_experts][hidden][inter] int8 (this rank's columns), [n_experts][hidden] fp32 */
} vh_mixtral_experts_i8;
/* vh_mixtral_create with int8 experts: `experts` is a host array of cfg->n_layers entries (copied); layers[l].w1 / w3 / w2 must
 * be null.  NULL (vh_last_error says why; VH_E_ARG) for a null array, a non-null bf16 expert pointer or a null int8 weight or
 * scale.  The workspace is vh_mixtral_workspace_bytes(cfg), as for the bf16 engine. */
vh_mixtral_t* vh_mixtral_create_i8(const vh_mixtral_cfg* cfg, const vh_mixtral_layer* layers, const vh_mixtral_experts_i8* experts,
                                   const uint16_t* embed, const float* final_norm, const uint16_t* lm_head, const float* rope_cos,
                                   const float* rope_sin, void* workspace, size_t workspace_bytes);
/* Per-row int8 quantisation (the formula above, IEEE divisions): w bf16 [rows][ld_src] -> s fp32 [rows] over all `cols`, and
 * q int8 [rows][ld_dst] holding columns [col0, col0 + ncols) (a TP rank's slice of w2 with the full-row scale). */
int vh_quant_rows_i8(const uint16_t* w, long rows, int cols, long ld_src, int col0, int ncols, int8_t* q, long ld_dst, float* s,
                     void* stream);
/* MXFP4 experts (quantization="experts_mxfp4"): OCP MXFP4 along K, the contiguous dimension, in blocks of 32
 * consecutive elements of a row.  amax = the block's largest |w|; se = max(floor(log2 amax) - 2, -125) (0 for a zero block); the
 * E8M0 scale byte is se + 127; v = w / 2^se saturates at +-6 and rounds to the nearest of 0, .5, 1, 1.5, 2, 3, 4, 6 (ties to the
 * even code); code = sign << 3 | index with the sign bit only for a non-zero magnitude.  The engine computes with
 * w' = e2m1(code) * 2^(byte - 127), which is a bf16 number.  Codes are uint8 [rows][K / 2] (element k in byte k >> 1, low nibble for
 * even k), scales uint8 [rows][K / 32].  A tensor-parallel rank's w2 column slice starts on a multiple of 32, so it stores the slice
 * of the codes and of the scales and every TP degree computes the same w'.  Activations stay fp32.  The contract covers scale
 * bytes 2 to 252, which is what the quantiser emits plus the range in which every w' is a normal bf16 number; other bytes are
 * outside it. */
typedef struct {
    const uint8_t* w1; const uint8_t* s1;   /* [n_experts][inter][hidden / 2] codes, [n_experts][inter][hidden / 32] scales */
    const uint8_t* w3; const uint8_t* s3;   /* as w1 / s1 */
    const uint8_t* w2; const uint8_t* s2;   /* [n_experts][hidden][inter / 2] codes, [n_experts][hidden][inter / 32] scales (this rank's columns) */
} vh_mixtral_experts_mxfp4;
/* vh_mixtral_create with MXFP4 experts: `experts` is a host array of cfg->n_layers entries (copied); layers[l].w1 / w3 / w2 must
 * be null.  NULL (vh_last_error says why; VH_E_ARG) for a null array, a non-null bf16 expert pointer, a null code or scale pointer,
 * or hidden / inter not a multiple of 64.  The workspace is vh_mixtral_workspace_bytes(cfg), as for the bf16 engine. */
vh_mixtral_t* vh_mixtral_create_mxfp4(const vh_mixtral_cfg* cfg, const vh_mixtral_layer* layers,
                                      const vh_mixtral_experts_mxfp4* experts, const uint16_t* embed, const float* final_norm,
                                      const uint16_t* lm_head, const float* rope_cos, const float* rope_sin, void* workspace,
                                      size_t workspace_bytes);
/* MXFP4 quantisation (the formula above): w bf16 [rows][ld_src], columns [col0, col0 + ncols) (both multiples of 32; ld_src % 8 == 0,
 * w 16-byte aligned) -> codes [rows][ld_codes_bytes] (ncols / 2 bytes written per row; ld_codes_bytes % 4 == 0) and scales
 * [rows][ld_scales] (ncols / 32 per row).  Inputs are finite. */
int vh_quant_mxfp4(const uint16_t* w, long rows, int cols, long ld_src, int col0, int ncols, uint8_t* codes, long ld_codes_bytes,
                   uint8_t* scales, long ld_scales, void* stream);
void vh_mixtral_destroy(vh_mixtral_t* m);

/* Tensor-parallel all-reduce hook (sum, fp32, in place).  Either the built-in RCCL path or a
 * caller-supplied callback (e.g. torch.distributed).  Unused when tp_world == 1. */
typedef int (*vh_allreduce_fn)(void* user, float* buf, long count, void* stream);
int vh_mixtral_set_allreduce(vh_mixtral_t* m, vh_allreduce_fn fn, void* user);
int vh_rccl_unique_id(void* out_128_bytes /* host */);
int vh_mixtral_init_rccl(vh_mixtral_t* m, const void* unique_id_128_bytes /* host */);

/* Prefill S embedded tokens at positions [pos0, pos0+S); leaves the first generated token in
 * out_tokens[0] (greedy) and the engine ready to decode.  If logits_out != NULL the fp32
 * logits of the last position are copied there ([vocab]).  hidden_dbg (nullable): fp32
 * [n_layers][S][hidden] receives the residual stream after every layer.                   */
/* ---- the library's own all-reduce over IPC-mapped peer buffers (vh_comm.hip): one process per GPU ------------------
 * vh_comm_create allocates this rank's receive buffer (the ONLY allocation the library makes: it must be fine-grained
 * device memory) and writes its 64-byte IPC handle to handle_out; the caller gathers the world's handles (any bootstrap:
 * torch.distributed, MPI, a file) and passes them, rank-major, to vh_comm_connect.  vh_comm_allreduce sums `count` fp32
 * values in place across the ranks (every rank must call it, in the same order, with the same count); results are
 * bit-identical on all ranks.  vh_comm_status: 0, or the phase whose bounded spin timed out (sticky: once set, every
 * later poll gives up at once).  vh_comm_create FAILS when fine-grained memory cannot be allocated, unless the caller
 * declared that all ranks share one device (vh_tune("comm_allow_coarse", 1): same-device tests); it reads
 * vh_tune("comm_ranks_per_device", n) — how many ranks drive this rank's device (1 on a node with a GPU per rank).  The 32-bit
 * granule tag wraps every 2^32 calls; the library then re-zeroes its regions between two barriers (collective, same call on all ranks).
 * vh_comm_create_loopback: a connected single-process communicator in which `rank` plays all `world` ranks into its own receive slots
 * (the stores, polls, tags and rank-ordered sums of a real exchange without a link; sums equal the inputs) — what
 * `bench.py --emulate-tp N --loopback` attaches to put the 65 exchanges of a decode step into one rank's measured time.
 * cap_elems <= 32768 (decode-sized messages only). */
typedef struct vh_comm vh_comm_t;
vh_comm_t* vh_comm_create(int rank, int world, size_t cap_elems, void* handle_out);
vh_comm_t* vh_comm_create_loopback(int rank, int world, size_t cap_elems);
int vh_comm_connect(vh_comm_t* c, const void* handles);
size_t vh_comm_capacity(const vh_comm_t* c);
int vh_comm_allreduce(vh_comm_t* c, float* buf, long count, void* stream);
int vh_comm_status(vh_comm_t* c);
void vh_comm_destroy(vh_comm_t* c);
const char* vh_comm_last_error(void);
int vh_comm_is_fine_grained(const vh_comm_t* c);              /* 1: the receive buffer is peer-coherent (required across devices) */
int vh_comm_debug_set_calls(vh_comm_t* c, uint64_t calls);    /* tests: continue from this call count on EVERY rank (tag wrap at 2^32) */
/* Route the engine's per-layer all-reduces through `c` (messages above its capacity keep using the RCCL / callback
 * collective installed before); null detaches it.  The engine does not own `c`. */
int vh_mixtral_use_comm(vh_mixtral_t* m, vh_comm_t* c);

/* Debug / parity hook: the top-2 expert ids of every layer of the following prefills are copied to ids_out
 * (device int[n_layers][S][2]; null switches it off) — SURVEY 8(c) golden list "router top-2 ids per layer". */
/* Give up on a vh_mixtral_init_rccl that is still running in another thread (bring-up time-out): when it returns it
 * destroys its communicator instead of installing it. */
int vh_mixtral_cancel_rccl(vh_mixtral_t* m);
int vh_mixtral_route_debug(vh_mixtral_t* m, int* ids_out);
int vh_mixtral_prefill(vh_mixtral_t* m, const float* embeds, int S, int pos0, float* logits_out, float* hidden_dbg,
                       void* stream);
/* Run n_steps greedy decode steps back to back with no host interaction.  Three launches per layer: the ATTENTION BLOCK as one
 * launch (k_dec_ablk: the fused-QKV rows, the split-KV attention tiles and the O-projection rows are work items of 2 persistent
 * blocks per CU; q|k|v and the attention output travel between items as tagged 8-byte granules, an item's weights / K-V tile are
 * in flight while it waits for its input; vh_tune("dec_fused", 0) runs it as three launches with the same arithmetic, bit for
 * bit), the router + gate|up GEMV of the two chosen experts, and the down projection.  Under tensor parallelism the two
 * all-reduces of a layer are fused into these launches (producer rows push to the peers, the first blocks of the consumer sum in
 * rank order: vh_tune("tp_fuse", 1), what ranks that own their device vote for) or run as one small kernel each.
 * Replaces the per-token forward of HF MixtralDecoderLayer x L as reached from vita/model/language_model/vita_mixtral.py:158-173. */
int vh_mixtral_decode(vh_mixtral_t* m, int n_steps, void* stream);
/* attention block of the last decode call: -1 none yet, 0 three launches (QKV, attention, O projection), 1 one fused launch. */
int vh_mixtral_decode_schedule(const vh_mixtral_t* m);
/* Device pointers into the engine state (for the host loop and the tests). */
const int* vh_mixtral_tokens(const vh_mixtral_t* m);     /* int[max_new]: generated ids   */
const int* vh_mixtral_counters(const vh_mixtral_t* m);   /* int[4]: {pos, n_generated, attn hand-off counter, device error flag (0 = ok)} */
const float* vh_mixtral_logits(const vh_mixtral_t* m);   /* fp32[max(1,logit_rows)][vocab]; row i = scores that produced token i */
int vh_mixtral_reset(vh_mixtral_t* m, void* stream);     /* n_generated = 0, pos = 0; frees every sequence and drops every page hold */
/* ---- concurrent sequences over a paged KV cache: what the reference's serving plugin receives from vLLM as
 * `kv_caches` + `attn_metadata` block tables (web_demo/vllm_tools/vllm_file/mixtral.py:491-501,1130-1186; the engine
 * that schedules them: web_interactive_demo.py:942-996).  The KV pool is cut into 64-token pages; a sequence is a slot
 * with its own page table (grown on demand), residual state, counters and generated ids.  A sequence's arithmetic is
 * exactly the single-sequence path's (same kernels, physical rows looked up through the table), so its ids and scores
 * do not depend on what else is scheduled.  Not to be mixed with vh_mixtral_prefill/decode while sequences are live.
 *   seq_alloc   -> slot id >= 0, or VH_E_FULL
 *   seq_prefill    appends S embedded tokens at the sequence's current position and leaves its next greedy token in
 *                  seq_tokens[0] (n_generated restarts at 0, as vh_mixtral_prefill); VH_E_FULL when pages run out
 *   seq_prefill_batch  the same for several sequences in one pass over the weights (below)
 *   seq_decode     one greedy step for each listed sequence, in order, on `stream` (a continuous-batching iteration)
 *   seq_free       returns the pages;  vh_mixtral_reset frees every sequence */
int vh_mixtral_seq_alloc(vh_mixtral_t* m);
int vh_mixtral_seq_free(vh_mixtral_t* m, int seq);
int vh_mixtral_seq_prefill(vh_mixtral_t* m, int seq, const float* embeds, int S, float* logits_out, void* stream);
int vh_mixtral_seq_decode(vh_mixtral_t* m, const int* seqs /* host */, int n, void* stream);
/* seq_prefill for n distinct live sequences in ONE pass over the weights (what vLLM's scheduler does with the prompts of queued
 * requests up to max_num_batched_tokens; here the bound is max_prefill).  embeds: device fp32 [sum(lens)][hidden], the segments'
 * rows back to back in list order.  Segment i appends lens[i] tokens at sequence seqs[i]'s current position (0 for a new sequence,
 * > 0 for a later chunk or turn) and leaves that sequence's next token in its seq_tokens[0] (n_generated restarts at 0), drawn with
 * THAT sequence's sampling parameters.  logits_out (nullable): device fp32 [n][vocab], row i = the scores of segment i's last
 * position.  Afterwards the state is what n vh_mixtral_seq_prefill calls in list order leave.
 *   The WHOLE call is checked before anything is enqueued or allocated: 1 <= n <= max_seqs, every slot live and not poisoned, no
 * slot twice, every lens[i] >= 1, sum(lens) <= max_prefill, every position + lens[i] < max_ctx; VH_E_FULL when the pool cannot
 * hold all segments (vh_mixtral_pages_free and every vh_mixtral_seq_pos are then what they were).  A failure after the first
 * enqueue poisons exactly the listed sequences.  n == 1 IS vh_mixtral_seq_prefill.
 *   Numerics: the rows of a sequence go through the same kernels and the same per-row arithmetic as alone, but not necessarily in
 * the same fp32 summation order (the K split of the projections is chosen on the device from the tile count of the pass, the
 * attention launcher picks its kernel from the launch size — as for batched decode iterations).  Ids and scores of a sequence
 * agree with the fp32 oracle of THAT SEQUENCE ALONE within the project's bar (ids equal, scores atol 1e-3); they are not
 * bit-identical with the one-by-one path.  K / V tile images stay a feature of the one-segment pass. */
int vh_mixtral_seq_prefill_batch(vh_mixtral_t* m, const int* seqs /* host */, const int* lens /* host */, int n,
                                 const float* embeds, float* logits_out, void* stream);
/* A MIXED pass (vLLM's enable_chunked_prefill: the next token of every running sequence rides as one extra row in the pass that
 * prefills the new prompts; what it replaces is the pair of a vh_mixtral_seq_prefill_batch call and the vh_mixtral_seq_decode
 * iteration behind it - two passes over the weights).  The rows of the pass are the prefill segments back to back (embeds: device
 * fp32 [sum(pf_lens)][hidden]; nullable when n_pf == 0), then one row per decode member: the embedding the last select left in that
 * sequence's state.  Segment i behaves exactly as in vh_mixtral_seq_prefill_batch (first token in seq_tokens[0], n_generated
 * restarts at 0); every sequence of dec_seqs advances ONE step exactly as vh_mixtral_seq_decode would advance it: its token is
 * appended, its position, draw index, penalty table and logprob rows go on (its counters are NOT reset).  A prompt longer than the
 * caller's row budget goes in as chunks over consecutive calls; only the last chunk's token counts.  logits_out (nullable): device
 * fp32 [n_pf + n_dec][vocab], rows in list order (prefill segments' last positions, then the decode rows).
 *   The WHOLE call is checked before anything is enqueued or allocated: n_pf + n_dec in [1, max_seqs], every slot live, not poisoned
 * and listed once across BOTH lists, every pf_lens[i] >= 1, sum(pf_lens) + n_dec <= max_prefill, every position + rows < max_ctx,
 * decode members have a prompt (position >= 1); VH_E_FULL when the pool cannot hold all members (vh_mixtral_pages_free and every
 * vh_mixtral_seq_pos are then what they were).  A failure after the first enqueue poisons exactly the listed sequences.
 * n_dec == 0 IS vh_mixtral_seq_prefill_batch; n_pf == 0 is a decode-only pass (the batched iteration's streaming MoE with the
 * projections on the GEMM too).
 *   The single rows' attention: the split-KV row kernels of vh_attn_rows at head_dim 128 with up to 4 query heads per KV head
 * (vh_tune("step_attn", 0), or another geometry: 1-row segments of the prefill's segment attention).
 *   Numerics: every row sees the project's exact-mode arithmetic - bf16 hi + lo planes in the GEMMs (the expert formats unchanged),
 * fp32 attention for the single rows.  Ids and scores of a sequence agree with the fp32 oracle of THAT SEQUENCE ALONE within the
 * project's bar (ids equal, scores atol 1e-3); a decode member is not bit-identical with vh_mixtral_seq_decode (GEMM instead of GEMV
 * summation order).  K / V tile images stay a feature of the one-segment pass. */
int vh_mixtral_seq_step(vh_mixtral_t* m, const int* pf_seqs /* host */, const int* pf_lens /* host */, int n_pf, const float* embeds,
                        const int* dec_seqs /* host */, int n_dec, float* logits_out, void* stream);
int vh_mixtral_pages_free(const vh_mixtral_t* m);
int vh_mixtral_seq_pos(const vh_mixtral_t* m, int seq);                  /* tokens in the sequence's KV cache, -1 = not live */
const int* vh_mixtral_seq_tokens(const vh_mixtral_t* m, int seq);        /* device int[max_new]  */
const int* vh_mixtral_seq_counters(const vh_mixtral_t* m, int seq);      /* device int[4], as vh_mixtral_counters */
int vh_mixtral_seq_table(const vh_mixtral_t* m, int seq, int* pages_out /* host */, int cap);   /* -> number of pages */
/* ---- shared pages: prefix caching over the block tables (vLLM's enable_prefix_caching; what it replaces is the plugin's use of
 * vLLM's block tables, web_demo/vllm_tools/vllm_file/mixtral.py:491-501, where a cached block appears in several tables).
 * Every page has a reference count in host memory: a sequence that has the page in its table counts 1, every HOLD counts 1.  A page
 * is on the free list exactly when its count is 0, and vh_mixtral_pages_free is the number of such pages.  While none of the entries
 * below is called, pages are handed out and returned in exactly the order they were before these entries existed.
 *   INVARIANT: the engine never writes a row of a page whose count is above 1 - adoption starts a sequence on a page boundary, holds
 * cover only full pages below the owner's position, and a sequence only writes at or above its own position.
 *   Each entry checks the WHOLE call before it changes anything and answers VH_E_ARG (text in vh_last_error) on a violation.  They are
 * host calls; tensor-parallel ranks make them with the same arguments.
 *   seq_hold_prefix  one more hold on each of the first n_pages (>= 1) pages of a live, unpoisoned sequence; their ids go to
 *                    pages_out.  Requires 64 * n_pages <= vh_mixtral_seq_pos(seq): only pages in which every position is written.
 *   pages_release    drops one count from each listed page (a page listed k times needs a count >= k).  Pages that reach 0 return to
 *                    the free list LAST LISTED FIRST, i.e. in the order seq_free returns a table: releasing the list seq_hold_prefix
 *                    gave, after the sequence was freed, leaves the free list as seq_free alone would have left it.
 *   seq_adopt        a live sequence at position 0 without pages takes the n (>= 1) listed pages as the first entries of its table, one
 *                    count each; table and position (64 * n: host mirror and device counters[0]) are uploaded on `stream`.  Every
 *                    page must have a count >= 1, none listed twice, n <= the table's capacity, 64 * n + 1 < max_ctx.  The next
 *                    seq_prefill / seq_prefill_batch segment of the sequence appends at 64 * n; work enqueued on `stream` earlier -
 *                    the prefill that wrote the pages - is ordered before it.
 *   page_refs        the count, -1 for a bad index.
 * seq_free drops the sequence's count of each of its pages; vh_mixtral_reset does that for every sequence and ALSO drops every hold
 * (the pool is one; pages that were only held return highest id first).  vh_mixtral_prefill / vh_mixtral_decode address the pool as
 * contiguous rows and answer VH_E_ARG while any page has a count > 0. */
int vh_mixtral_seq_hold_prefix(vh_mixtral_t* m, int seq, int n_pages, int* pages_out /* host */);
int vh_mixtral_pages_release(vh_mixtral_t* m, const int* pages /* host */, int n);
int vh_mixtral_seq_adopt(vh_mixtral_t* m, int seq, const int* pages /* host */, int n, void* stream);
int vh_mixtral_page_refs(const vh_mixtral_t* m, int page);

/* ---- batch-1 decode operators, one entry per kernel group ---------------------------------------------------
 * The steps vh_mixtral_decode chains inside one HF MixtralDecoderLayer (third-party modeling_mixtral.py, reached from
 * vita/model/language_model/vita_mixtral.py:158-169), exposed one by one so that a single module can be bound.  All
 * scratch is the caller's.
 *
 * vh_router_top2 (K25): MixtralSparseMoeBlock's gate on ALREADY NORMED rows — logits = x Wg^T, fp32 softmax, top-2,
 *   renormalise (web_demo/vllm_tools/vllm_file/mixtral.py:398-411, renormalize=True).  x fp32 [rows][ldx], Wg bf16 [E][H],
 *   ids int[rows][2], wts fp32 [rows][2], probs (nullable) fp32 [rows][E].                                                */
int vh_router_top2(const float* x, long ldx, const uint16_t* Wg, int E, int H, int rows, int* ids, float* wts, float* probs,
                   void* stream);
/* vh_moe_decode (K20 + K25 + K26, one token): y = block_sparse_moe(post_attention_layernorm(x + delta)) — the second half
 *   of MixtralDecoderLayer.forward WITHOUT the residual add: RMSNorm (weight norm_w, eps), router as above, the two routed
 *   experts' w2(silu(w1 h) * w3 h) weighted and summed.  x, delta (nullable), y fp32 [H]; x_out (nullable) receives x + delta;
 *   W1, W3 bf16 [E][I][H], W2 bf16 [E][H][I]; route int[4] = {e0, e1, bits(w0), bits(w1)}; hbuf fp32 [2 I] scratch.          */
int vh_moe_decode(const float* x, const float* delta, const float* norm_w, float eps, const uint16_t* Wg, const uint16_t* W1,
                  const uint16_t* W3, const uint16_t* W2, int E, int I, int H, float* x_out, float* y, int* route, float* hbuf,
                  void* stream);
/* vh_moe_decode_i8: the same on int8 experts (vh_mixtral_experts_i8 layout; s1, s3 [E][I], s2 [E][H]); the router stays bf16. */
int vh_moe_decode_i8(const float* x, const float* delta, const float* norm_w, float eps, const uint16_t* Wg, const int8_t* W1,
                     const float* s1, const int8_t* W3, const float* s3, const int8_t* W2, const float* s2, int E, int I, int H,
                     float* x_out, float* y, int* route, float* hbuf, void* stream);
/* vh_moe_decode_mxfp4: the same on MXFP4 experts (vh_mixtral_experts_mxfp4 layout: codes and scale bytes); the router stays bf16. */
int vh_moe_decode_mxfp4(const float* x, const float* delta, const float* norm_w, float eps, const uint16_t* Wg, const uint8_t* W1,
                        const uint8_t* s1, const uint8_t* W3, const uint8_t* s3, const uint8_t* W2, const uint8_t* s2, int E, int I, int H,
                        float* x_out, float* y, int* route, float* hbuf, void* stream);
/* vh_rope_kv_append (K22): rotate-half RoPE on the q and k heads of S fused-QKV rows and append k, v to the cache at
 *   positions [pos0, pos0 + S) (HF apply_rotary_pos_emb + Cache.update; vLLM rotary_emb + KV write, mixtral.py:477-501).
 *   qkv fp32 [S][ldqkv] = q heads | k heads | v heads (head_dim 128); q_out fp32 [S][nq*128]; caches fp32
 *   [nkv][max_ctx][128]; rope_cos / rope_sin fp32 [max_pos][64]; table (nullable) = 64-row page table of a paged cache.      */
int vh_rope_kv_append(const float* qkv, long ldqkv, float* q_out, float* kcache, float* vcache, const float* rope_cos,
                      const float* rope_sin, int S, int pos0, int nq, int nkv, int max_ctx, const int* table, void* stream);
/* vh_attn_decode (K22 + K23, one token): RoPE(q, k_new), KV append at `pos`, causal GQA attention of the token against
 *   positions [0, pos] (MixtralAttention.forward between the projections).  qkv fp32 [(nq + 2 nkv) * 128]; attn_out fp32
 *   [nq * 128]; scratch: part_o fp32 [nq][ceil(max_ctx / 64)][128], part_ml fp32 [nq][ceil(max_ctx / 64)][2], tickets
 *   int[nkv] (zero before the first call; the kernel resets them).                                                           */
int vh_attn_decode(const float* qkv, float* kcache, float* vcache, int pos, const float* rope_cos, const float* rope_sin,
                   int nq, int nkv, int max_ctx, float scale, const int* table, float* part_o, float* part_ml, int* tickets,
                   float* attn_out, void* stream);
/* vh_attn_decode_batch: vh_attn_decode for n (1 ... 4) sequences of one paged K / V pool in ONE launch — the attention step of a
 *   batched decode iteration (vh_mixtral_seq_decode), per sequence the arithmetic of vh_attn_decode.  qkv, pos, table, part_o,
 *   part_ml, tickets and attn_out are HOST arrays of n entries: sequence b appends its token at pos[b] through its page table
 *   table[b] (entry nullable: the contiguous layout) and attends over [0, pos[b]].  Every sequence has its own scratch (sizes as
 *   for vh_attn_decode) and output; the sequences' pages must be disjoint.  VH_E_ARG: a null pointer, buffers shared between two
 *   sequences; VH_E_SHAPE: n outside [1, 4], a position outside the cache.  Nothing is launched on an error.                  */
int vh_attn_decode_batch(int n, const float* const* qkv, float* kcache, float* vcache, const int* pos, const float* rope_cos,
                         const float* rope_sin, int nq, int nkv, int max_ctx, float scale, const int* const* table,
                         float* const* part_o, float* const* part_ml, int* const* tickets, float* const* attn_out, void* stream);
/* vh_attn_rows: causal GQA attention of n SINGLE query rows whose q is already rotated, each against its own paged sequence - the
 *   attention of the decode rows of a mixed pass (vh_mixtral_seq_step).  It replaces, for such a row, a 16-row query tile of the
 *   prefill's segment attention (one block per KV head walking the whole context) and vh_attn_decode_batch (which wants un-rotated
 *   q|k|v of at most 4 sequences and appends K / V itself): here nothing is appended, row i attends over keys [0, klens[i]) that are
 *   in the pool already.  q fp32 row i at q + i * ldq = [nq][128]; pools fp32 [nkv][max_ctx][128] in 64-row pages; klens: HOST
 *   int[n]; tables: HOST array of n device page tables (ceil(klens[i] / 64) entries each).  Pool rows past a row's klens may hold
 *   anything.  Two launches: one (m, l, o) partial per (row, head, 64-key tile), then a merge in ascending tile order (no hand-off
 *   inside a launch).  Output row i: out fp32 [n][ldo] and / or the bf16 hi / lo planes out_hi / out_lo (same stride; hi + lo ~ the
 *   fp32 value, what vh_gemm_ps reads).  scratch: vh_attn_rows_scratch_bytes(n, nq, max klens) device bytes hold all rows in one
 *   launch pair; with less (at least the descriptors and one row) the rows run in several.  The descriptor upload is waited for.
 *   VH_E_ARG: a null or misaligned pointer; VH_E_SHAPE: klens outside [1, max_ctx], heads, strides, scratch too small.  Nothing is
 *   launched on an error.                                                                                                      */
size_t vh_attn_rows_scratch_bytes(int n, int nq, int max_klen);
int vh_attn_rows(int n, const float* q, long ldq, const float* kcache, const float* vcache, const int* klens /* host */,
                 const int* const* tables /* host */, int nq, int nkv, int max_ctx, float scale, void* scratch, size_t scratch_bytes,
                 float* out, uint16_t* out_hi, uint16_t* out_lo, long ldo, void* stream);
/* vh_lmhead_argmax (K27 + K28): logits = lm_head(norm(x + delta)) in fp32 (vita_mixtral.py:171-172) and their argmax
 *   (lowest index on ties, as torch.argmax in HF greedy search).  W bf16 [V][H]; logits fp32 [V]; token_out int[1];
 *   blk_val / blk_idx: nblk floats / ints of scratch (nblk = blocks of the launch, e.g. 1024).                               */
int vh_lmhead_argmax(const float* x, const float* delta, const float* norm_w, float eps, const uint16_t* W, int V, int H,
                     float* logits, int* token_out, float* blk_val, int* blk_idx, int nblk, void* stream);

/* ---- seeded sampling (replaces HF GenerationMixin sampling with its TemperatureLogitsWarper, TopKLogitsWarper and
 * TopPLogitsWarper — transformers generation/utils.py _sample, generation/logits_process.py — and vLLM's Sampler behind
 * SamplingParams(temperature, top_k, top_p, seed), web_demo/web_ability_demo.py:351) --------------------------------------
 * Per request: z = (double)logit / temperature; top-k keeps z >= the k-th largest z (ties kept); top-p, on the softmax of the
 * top-k-kept set, keeps a value iff the mass strictly above it is < top_p (the maximum always, ties together; masses in double);
 * the token is the argmax over kept i of z_i + G_i (lowest index on ties), G_i = -log(-log(u)), u = ((x >> 11) + 0.5) 2^-53,
 * x = word i & 3 of Philox4x64-10 under key (seed, 0) at counter (i >> 2, draw, 0, 0).  draw = draw0 + the token's index in the
 * request's output (the prefill's token is index 0), counted on the device.  Sampled candidates cross blocks and ranks as exact
 * keys of their double scores, so given the logits a token is a function of the request alone (not of the grid, the vocab
 * shards, the batch-mates or the lookahead window).
 * NaN logits rank as -inf; when nothing finite is kept the id is 0.  temperature = 0 (or a null vh_sampling) is greedy: the
 * greedy kernels and launches unchanged.  temperature must be finite and >= 0, top_k >= 0 (0 = off), 0 < top_p <= 1 (1 = off).
 * Under a vocab-sharded LM head (vocab_n > 0) only temperature-only sampling is accepted (VH_E_ARG otherwise); an unsharded head
 * under tensor parallelism holds the same logits on every rank, so every rank draws the same token. */
typedef struct {
    float temperature;
    int top_k;
    float top_p;
    uint64_t seed;
    int64_t draw0;
} vh_sampling;
/* single-sequence engine (vh_mixtral_prefill / decode); vh_mixtral_reset restores greedy */
int vh_mixtral_set_sampling(vh_mixtral_t* m, const vh_sampling* s /* host, nullable */);
/* one sequence of the paged engine; seq_alloc, seq_free and vh_mixtral_reset restore greedy */
int vh_mixtral_seq_set_sampling(vh_mixtral_t* m, int seq, const vh_sampling* s /* host, nullable */);
/* per-operator entry: tokens_out[r] = the draw of row r = logits + r * ld (ld = 0: the same row for every draw) at draw index
 *   draw0 + r, by the engine's device code.  logits fp32, V entries per row; tokens_out int[rows].                             */
int vh_sample_rows(const float* logits, long ld, int rows, int V, const vh_sampling* s /* host */, int* tokens_out, void* stream);

/* ---- logit rules: repetition / presence / frequency penalties and log-probabilities on the device (replaces HF
 * RepetitionPenaltyLogitsProcessor — transformers generation/logits_process.py — and vLLM's apply_penalties + Sampler logprobs behind
 * SamplingParams(repetition_penalty, presence_penalty, frequency_penalty, logprobs)) ----------------------------------------------
 * History of a request: P = the SET of its prompt ids, c[v] = how often id v occurs in its output so far (the prefill's token is
 * output 0).  The engine keeps both per request in a token table uint32 seen[vocab] (bit 31 = in P, low bits = c[v]) and counts every
 * token it writes on the device, so multi-step decode stays host-free.
 * Penalties: the fp32 logit x of id v becomes, each step a single IEEE fp32 operation without contraction, in this order
 *   1. v in P or c[v] > 0:  x = x > 0 ? x / r : x * r          (r = repetition_penalty)
 *   2.                      x = x - f * (float)c[v]            (f = frequency_penalty; a product, then a difference)
 *   3. c[v] > 0:            x = x - p                          (p = presence_penalty)
 * NaN stays NaN, +-inf follows IEEE.  The penalised value is what SELECTION sees (greedy argmax, the temperature-only Gumbel
 * compare, the top-k / top-p filter); the kept logits rows stay RAW, as under sampling.  r = 1, f = p = 0 is "off": a request with
 * neutral penalties and no logprobs launches exactly the kernels of an engine without rules.
 * Logprobs: logprobs = K, 0 <= K <= max_logprobs <= 20, gives every generated token the log-probability of the chosen id and the K
 * most probable ids with theirs, under log_softmax of the RAW fp32 logits row of that step (vLLM's default raw_logprobs, HF's
 * output_logits view): x_v - (M + log sum_j exp(x_j - M)) in double, M the row maximum, the sum taken as one partial per wave added
 * in wave order, rounded to fp32 once.  The top K are ordered by (logit descending, id ascending); entries past the vocabulary are
 * id -1 and -inf; NaN logits rank as -inf and a row with nothing finite gives -inf everywhere.  logprobs = -1 is off.
 * Accepted: finite r > 0, finite f and p, -1 <= logprobs <= cfg.max_logprobs; non-neutral penalties need cfg.penalty_tables,
 * logprobs >= 0 needs cfg.max_logprobs > 0.  Under a vocab-sharded LM head (vocab_n > 0) non-neutral penalties and logprobs are refused
 * (VH_E_ARG), as filters are; an unsharded head under tensor parallelism works unchanged (every rank holds the same row and table). */
typedef struct {
    float repetition_penalty, presence_penalty, frequency_penalty;
    int logprobs;
} vh_logit_rules;
/* Rules of the single-sequence engine (vh_mixtral_prefill / decode) from the next prefill on.  The table is cleared, ids[0, n_prompt)
 * are marked as prompt and ids[n_prompt, n_prompt + n_output) counted as outputs (how a recomputed sequence or a later turn gets its
 * history back); a call without penalties (rules == NULL: off, or logprobs only) leaves it all zero.  The whole call is validated
 * before anything changes: an id outside [0, vocab) or a bad value is VH_E_ARG and leaves the previous setting AND table in force.
 * A call that has to write the table — one with penalties, or the first one without after a request that had them — waits for the
 * device the workspace lives on (whichever device is current) and writes with a blocking copy; other calls touch nothing on the
 * device.  vh_mixtral_reset restores "off"; seq_alloc / seq_free / reset do not touch a table, the next setter call on that
 * engine / slot does. */
int vh_mixtral_set_logit_rules(vh_mixtral_t* m, const vh_logit_rules* rules /* host, nullable */, const int* ids /* host */,
                               int n_prompt, int n_output);
/* the same for one sequence of the paged engine; seq_alloc, seq_free and vh_mixtral_reset restore "off" */
int vh_mixtral_seq_set_logit_rules(vh_mixtral_t* m, int seq, const vh_logit_rules* rules /* host, nullable */,
                                   const int* ids /* host */, int n_prompt, int n_output);
/* Device pointers of the logprob buffers (null without cfg.max_logprobs): entry i belongs to generated token i of the current
 * (re)prefill, as vh_mixtral_tokens.  token: fp32 [max_new]; top_ids: int [max_new][max_logprobs]; top: fp32 [max_new][max_logprobs]
 * (the first K of a row are written). */
const float* vh_mixtral_logprobs_token(const vh_mixtral_t* m);
const int* vh_mixtral_logprobs_top_ids(const vh_mixtral_t* m);
const float* vh_mixtral_logprobs_top(const vh_mixtral_t* m);
const float* vh_mixtral_seq_logprobs_token(const vh_mixtral_t* m, int seq);
const int* vh_mixtral_seq_logprobs_top_ids(const vh_mixtral_t* m, int seq);
const float* vh_mixtral_seq_logprobs_top(const vh_mixtral_t* m, int seq);
const uint32_t* vh_mixtral_seen(const vh_mixtral_t* m);                 /* the token tables (null without cfg.penalty_tables) */
const uint32_t* vh_mixtral_seq_seen(const vh_mixtral_t* m, int seq);
/* per-operator entry: the engine's device code on caller-provided rows (row r = logits + r * ld, V entries).  seen (nullable, device
 * uint32[V]): one table for all rows; penalised_out (nullable, device fp32 [rows][V]) receives the penalised rows (rules->logprobs is
 * not read).  lp_tok (nullable; then tokens, and for K > 0 lp_top_id and lp_top, must be set): tokens[r] is the chosen id of row r,
 * lp_tok fp32 [rows], lp_top_id int [rows][K], lp_top fp32 [rows][K], 0 <= K <= 20, of the RAW rows. */
int vh_logit_rules_rows(const float* logits, long ld, int rows, int V, const vh_logit_rules* rules /* host */, const uint32_t* seen,
                        float* penalised_out, const int* tokens, float* lp_tok, int* lp_top_id, float* lp_top, int K, void* stream);

/* Live HIP-event timing of the dominant kernel of a phase, on the stream the engine launches it on: stride > 0 samples the
 * DECODE gate|up expert GEMV of every stride-th layer, stride < 0 the PREFILL gate|up grouped GEMM of every |stride|-th layer
 * (0 = off), up to max_samples launches; read returns summed ms and sample count and clears the samples. */
int vh_mixtral_profile(vh_mixtral_t* m, int stride, int max_samples);
int vh_mixtral_profile_read(vh_mixtral_t* m, double* total_ms /* host */, int* count /* host */);

#ifdef __cplusplus
}
#endif
#endif
