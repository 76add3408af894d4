// vh_elem.hip — HBM-bound row / index kernels around the GEMMs (SURVEY §2.4 K1-K3, K8,
// K11-K13, K18-K20, K22, K25).  All fp32 activations; small parameters (norm weights,
// biases) are fp32 arrays holding bf16-representable values, large tables are bf16.
#include "vh_common.h"
#include "vh_kernels.h"

namespace {

// ---- LayerNorm / RMSNorm: one wave per row, row cached in registers -------------------
// torch.nn.LayerNorm semantics (biased variance).  Optional activation and post-scale
// fuse Whale's embed tail  Linear -> LN -> ReLU -> x*sqrt(d)  (transformer.py:312-318,
// attention.py:108-111) and the adapter's LN -> GELU (adapter.py:128-133).
#define LN_MAXV 16  // float4 per lane -> cols <= 4096
template <bool RMS>
__global__ __launch_bounds__(256) void k_norm_rows(const float* __restrict__ x, long ldx, float* __restrict__ y,
                                                   long ldy, const float* __restrict__ w,
                                                   const float* __restrict__ b, int rows, int cols, float eps,
                                                   int act, float post_scale) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wid;
    if (row >= rows) return;
    const int nv = cols >> 2;
    const float4* xp = reinterpret_cast<const float4*>(x + (size_t)row * ldx);
    float4 v[LN_MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        const int c = lane + i * 64;
        if (c < nv) { v[i] = xp[c]; s += (v[i].x + v[i].y) + (v[i].z + v[i].w); }
        else v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float mean = 0.f;
    if (!RMS) mean = wave_sum(s) / (float)cols;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
            const float a = v[i].x - mean, bq = v[i].y - mean, cq = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + bq * bq) + (cq * cq + d * d);
        }
    }
    const float inv = rsqrtf(wave_sum(q) / (float)cols + eps);
    float4* yp = reinterpret_cast<float4*>(y + (size_t)row * ldy);
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
            const float4 ww = reinterpret_cast<const float4*>(w)[c];
            float4 r;
            r.x = (v[i].x - mean) * inv * ww.x; r.y = (v[i].y - mean) * inv * ww.y;
            r.z = (v[i].z - mean) * inv * ww.z; r.w = (v[i].w - mean) * inv * ww.w;
            if (b) {
                const float4 bb = reinterpret_cast<const float4*>(b)[c];
                r.x += bb.x; r.y += bb.y; r.z += bb.z; r.w += bb.w;
            }
            if (act != VH_ACT_NONE) {
                r.x = apply_act(r.x, act); r.y = apply_act(r.y, act);
                r.z = apply_act(r.z, act); r.w = apply_act(r.w, act);
            }
            r.x *= post_scale; r.y *= post_scale; r.z *= post_scale; r.w *= post_scale;
            yp[c] = r;
        }
    }
}

// ---- Mixtral prefill: post-attention RMSNorm fused with the top-2 router ------------------
// One 256-thread block per token: thread t owns the 16-byte chunks t + 256 j of the row, the sum of squares and
// the 8 router logits are one block reduction (9 values), thread 0 does the fp32 softmax / top-2 / renormalise
// (modeling_mixtral.py:96-111; ties resolve to the lowest expert index like torch.topk).  The normalised row
// is written as fp32 and/or as the bf16 hi/lo planes the weight-streaming MoE GEMM consumes (x = hi + lo to
// 2^-17), so no separate split pass runs.  (Round 1 used one WAVE per row with a serial 8-expert FMA chain:
// 138 blocks, 75 us for a 9 MB read; this shape is 552 blocks x 128 FMAs per thread.)
#define RR_MAXJ 4   // chunks per thread -> cols <= 4096
// UPD (r03): the row first takes the update its producer left as K-split slabs (VhRowUpdate: the O projection's slabs
// before the FFN norm, the previous layer's expert outputs before the attention norm) and is written back — the
// arithmetic and its order are those of k_sum_slabs / k_moe_combine, which this replaces on the prefill path.
template <int UPD>
__global__ __launch_bounds__(256) void k_rmsnorm_route(float* __restrict__ x, float* __restrict__ y,
                                                       uint16_t* __restrict__ y_hi, uint16_t* __restrict__ y_lo,
                                                       const float* __restrict__ w, int rows, int cols, float eps,
                                                       const uint16_t* __restrict__ Wg, int E,
                                                       int* __restrict__ ids, float* __restrict__ wts, const VhRowUpdate u) {
    __shared__ float red[4 * 9];
    const int row = blockIdx.x;
    const int nv = cols >> 2;
    f32x4* xp = reinterpret_cast<f32x4*>(x + (size_t)row * cols);
    f32x4 v[RR_MAXJ], g[RR_MAXJ];
#pragma unroll
    for (int j = 0; j < RR_MAXJ; ++j) {
        const int c = threadIdx.x + j * 256;
        const int cc = c < nv ? c : 0;
        v[j] = xp[cc];
        g[j] = reinterpret_cast<const f32x4*>(w)[cc];
        if (c >= nv) v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (UPD != 0) {
        const int ns = u.nslab_dev ? *u.nslab_dev : u.nslab;
        if (UPD == 1) {
            const f32x4* sp = reinterpret_cast<const f32x4*>(u.src + (size_t)row * u.ld);
#pragma unroll
            for (int j = 0; j < RR_MAXJ; ++j) {
                const int c = threadIdx.x + j * 256;
                if (c >= nv) continue;
                f32x4 a = sp[c];
                for (int k = 1; k < ns; ++k) a += *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(sp + c) + (size_t)k * u.stride);
                v[j] = a + v[j];
                xp[c] = v[j];
            }
        } else {
            const float w0 = u.wts[row * 2], w1 = u.wts[row * 2 + 1];
            const f32x4* s0 = reinterpret_cast<const f32x4*>(u.src + (size_t)(2 * row) * u.ld);
            const f32x4* s1 = reinterpret_cast<const f32x4*>(u.src + (size_t)(2 * row + 1) * u.ld);
#pragma unroll
            for (int j = 0; j < RR_MAXJ; ++j) {
                const int c = threadIdx.x + j * 256;
                if (c >= nv) continue;
                f32x4 y0 = s0[c], y1 = s1[c];
                for (int k = 1; k < ns; ++k) {
                    y0 += *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(s0 + c) + (size_t)k * u.stride);
                    y1 += *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(s1 + c) + (size_t)k * u.stride);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) v[j][i] += w0 * y0[i] + w1 * y1[i];
                xp[c] = v[j];
            }
        }
    }
    float vals[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) vals[e] = 0.f;
#pragma unroll
    for (int j = 0; j < RR_MAXJ; ++j) {
        vals[8] += (v[j][0] * v[j][0] + v[j][1] * v[j][1]) + (v[j][2] * v[j][2] + v[j][3] * v[j][3]);
        v[j] = v[j] * g[j];                               // x * w_norm; the scalar 1/rms commutes with the dot products
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (e < E) {
#pragma unroll
            for (int j = 0; j < RR_MAXJ; ++j) {
                const int c = threadIdx.x + j * 256;
                const uint2 q = reinterpret_cast<const uint2*>(Wg + (size_t)e * cols)[c < nv ? c : 0];
                float a = vals[e];
                a = fmaf(v[j][0], bf16_lo_to_f32(q.x), a);
                a = fmaf(v[j][1], bf16_hi_to_f32(q.x), a);
                a = fmaf(v[j][2], bf16_lo_to_f32(q.y), a);
                a = fmaf(v[j][3], bf16_hi_to_f32(q.y), a);
                vals[e] = a;                              // chunks past the row hold v = 0
            }
        }
    }
    block256_sum<9>(vals, red);
    const float inv = rsqrtf(vals[8] / (float)cols + eps);
#pragma unroll
    for (int j = 0; j < RR_MAXJ; ++j) {
        const int c = threadIdx.x + j * 256;
        if (c < nv) {
            const f32x4 r = v[j] * inv;
            if (y) reinterpret_cast<f32x4*>(y + (size_t)row * cols)[c] = r;
            if (y_hi) {
                uint32_t hi[2], lo[2];
                split_bf16_pair(r[0], r[1], hi[0], lo[0]);
                split_bf16_pair(r[2], r[3], hi[1], lo[1]);
                reinterpret_cast<uint2*>(y_hi + (size_t)row * cols)[c] = make_uint2(hi[0], hi[1]);
                reinterpret_cast<uint2*>(y_lo + (size_t)row * cols)[c] = make_uint2(lo[0], lo[1]);
            }
        }
    }
    if (threadIdx.x == 0 && E > 0) {
        float lg[8];
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) { lg[e] = vals[e] * inv; if (e < E) mx = fmaxf(mx, lg[e]); }
        float pr[8], sum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { pr[e] = (e < E) ? expf(lg[e] - mx) : 0.f; sum += pr[e]; }
        int e0 = 0, e1 = 0;
        float b0 = -1.f, b1 = -1.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { pr[e] /= sum; if (e < E && pr[e] > b0) { b0 = pr[e]; e0 = e; } }
#pragma unroll
        for (int e = 0; e < 8; ++e) if (e < E && e != e0 && pr[e] > b1) { b1 = pr[e]; e1 = e; }
        const float t = b0 + b1;
        ids[row * 2] = e0; ids[row * 2 + 1] = e1;
        wts[row * 2] = b0 / t; wts[row * 2 + 1] = b1 / t;
    }
}

__global__ void k_add(float* __restrict__ x, const float* __restrict__ y, long n4) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        float4 a = reinterpret_cast<float4*>(x)[i];
        const float4 b = reinterpret_cast<const float4*>(y)[i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        reinterpret_cast<float4*>(x)[i] = a;
    }
}

// x[r, :] += [a[r, :] | b[r, :]]  (a, b: the two column halves [rows][cols/2] of the overlapped TP prefill)

// ---- content digests of 64-row blocks (vh_hash_row_blocks, include/vita_hip.h): lane j of block b is
// fmix32(sum_i fmix32(word_i ^ fmix32(4 i + j + GOLD)) + (j + 1) GOLD), i = position of the word inside the block.  Every reduction
// step is a wrapping add, so neither the split of a block over workgroups nor the order of the atomics shows in the result.
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {   // MurmurHash3's 32-bit finaliser (a bijection)
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
constexpr uint32_t HASH_GOLD = 0x9E3779B9u;
constexpr int HASH_ROWS_PER_WG = 2;   // 32 workgroups per 64-row block: S = 2344 (36 blocks) puts 1152 workgroups on 256 CUs
__device__ __forceinline__ void hash_word(uint32_t w, uint32_t i, uint32_t (&acc)[4]) {
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) acc[j] += fmix32(w ^ fmix32(4u * i + j + HASH_GOLD));
}
// grid (64 / HASH_ROWS_PER_WG, blocks); VEC: rows are 16-byte aligned and cols % 4 == 0 (one 16-byte load per four words)
template <bool VEC>
__global__ void __launch_bounds__(256) k_hash_row_blocks(const float* __restrict__ x, long ldx, int cols, uint32_t* __restrict__ out) {
    const int blk = blockIdx.y, r0 = blockIdx.x * HASH_ROWS_PER_WG;
    const float* base = x + ((long)blk * 64 + r0) * ldx;
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    if (VEC) {
        const int c4n = cols / 4;
        for (int t = threadIdx.x; t < HASH_ROWS_PER_WG * c4n; t += 256) {
            const int r = t / c4n, c = (t - r * c4n) * 4;
            const uint4 v = *reinterpret_cast<const uint4*>(base + (long)r * ldx + c);
            const uint32_t i = (uint32_t)(r0 + r) * (uint32_t)cols + (uint32_t)c;
            hash_word(v.x, i, acc); hash_word(v.y, i + 1, acc); hash_word(v.z, i + 2, acc); hash_word(v.w, i + 3, acc);
        }
    } else {
        for (int t = threadIdx.x; t < HASH_ROWS_PER_WG * cols; t += 256) {
            const int r = t / cols, c = t - r * cols;
            hash_word(__float_as_uint(base[(long)r * ldx + c]), (uint32_t)(r0 + r) * (uint32_t)cols + (uint32_t)c, acc);
        }
    }
    // wave sums, then the workgroup's four lane sums through LDS: one 16-byte group of atomics per workgroup
    __shared__ uint32_t part[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t v = acc[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_down((int)v, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4)
        atomicAdd(out + (long)blk * 4 + threadIdx.x, part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}
__global__ void k_hash_finish(uint32_t* __restrict__ out, int n) {   // n = 4 * blocks
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = fmix32(out[t] + (uint32_t)((t & 3) + 1) * HASH_GOLD);
}

// dst (+)= sum of the K-split partial slabs of a projection (slab k at src + k * stride; count read on the device)
__global__ void k_sum_slabs(float* __restrict__ dst, long ldd, const float* __restrict__ src, long lds, int rows, int cols4,
                            const int* __restrict__ nslab_dev, int nslab, long stride, int accumulate) {
    const int ns = nslab_dev ? *nslab_dev : nslab;
    const long total = (long)rows * cols4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols4;
        const int c = (int)(i - r * cols4);
        const float4* sp = reinterpret_cast<const float4*>(src + r * lds) + c;
        float4 a = *sp;
        for (int k = 1; k < ns; ++k) {
            const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(sp) + (size_t)k * stride);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        float4* dp = reinterpret_cast<float4*>(dst + r * ldd) + c;
        if (accumulate) { const float4 o = *dp; a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w; }
        *dp = a;
    }
}
__global__ void k_add_halves(float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ b, int rows,
                             int cols4) {
    const long total = (long)rows * cols4;
    const int h4 = cols4 / 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols4;
        const int c = (int)(i - r * cols4);
        const float4 v = c < h4 ? reinterpret_cast<const float4*>(a)[r * h4 + c] : reinterpret_cast<const float4*>(b)[r * h4 + c - h4];
        float4 o = reinterpret_cast<float4*>(x)[i];
        o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
        reinterpret_cast<float4*>(x)[i] = o;
    }
}

__global__ void k_cast_bf16_f32(const uint16_t* __restrict__ in, float* __restrict__ out, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = bf16_to_f32(in[i]);
}

// ---- InternViT front/back ends --------------------------------------------------------
// patchify: conv 14x14 stride 14 as a GEMM row: out[(img,py,px), c*P*P + ky*P + kx]
// (modeling_intern_vit.py:80-85,109-111); columns >= 3*P*P are zero padding (K % 64).
__global__ void k_vit_patchify(const float* __restrict__ pix, float* __restrict__ out, int n, int img, int patch,
                               int kpad) {
    const int g = img / patch;
    const long total = (long)n * g * g * kpad;
    const int kk = 3 * patch * patch;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % kpad);
        const long row = i / kpad;
        float v = 0.f;
        if (k < kk) {
            const int c = k / (patch * patch), rem = k % (patch * patch);
            const int ky = rem / patch, kx = rem % patch;
            const int px = (int)(row % g), py = (int)((row / g) % g), im = (int)(row / ((long)g * g));
            v = pix[(((long)im * 3 + c) * img + (py * patch + ky)) * img + px * patch + kx];
        }
        out[i] = v;
    }
}

// embeddings = cat([cls, patch_embeds]) + position_embedding (modeling_intern_vit.py:112-121;
// the bicubic pos-embed resize is the identity at 448/14 = the trained 32x32 grid).
__global__ void k_vit_assemble(const float* __restrict__ patches, const uint16_t* __restrict__ cls,
                               const uint16_t* __restrict__ pos, float* __restrict__ x, int n, int ntok, int hid) {
    const long total = (long)n * ntok * hid;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % hid);
        const int t = (int)((i / hid) % ntok);
        const long im = i / ((long)hid * ntok);
        const float base = (t == 0) ? bf16_to_f32(cls[c]) : patches[((long)im * (ntok - 1) + (t - 1)) * hid + c];
        x[i] = base + bf16_to_f32(pos[(long)t * hid + c]);
    }
}

// drop CLS, x0.5, pixel_shuffle(0.5): out[n, a*g2+b, e] = mul * x[n, 1 + d1*g + d2, c] with
// d1 = 2a + e/(2C), d2 = 2b + (e%(2C))/C, c = e%C   (internvit_encoder.py:35-53,71-77)
__global__ void k_vit_pixel_shuffle(const float* __restrict__ x, float* __restrict__ out, int n, int g, int C,
                                    float mul) {
    const int g2 = g / 2;
    const long total = (long)n * g2 * g2 * 4 * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int e = (int)(i % (4 * C));
        const long t = i / (4 * C);
        const int bb = (int)(t % g2), a = (int)((t / g2) % g2);
        const long im = t / ((long)g2 * g2);
        const int d1 = 2 * a + e / (2 * C), d2 = 2 * bb + (e % (2 * C)) / C, c = e % C;
        out[i] = mul * x[((long)im * (g * g + 1) + 1 + d1 * g + d2) * C + c];
    }
}

// ---- Whale front end: GlobalCMVN + Conv2d(1,C,3,2) + ReLU, channels-last output ---------
// out[t1, f1, c] = relu(b[c] + sum_{kh,kw} w[c,kh,kw] * ((x[2t1+kh, 2f1+kw] - mean)*istd))
// (cmvn.py:29-32, subsampling.py:28-31)
// B clips of a common padded length T, clip after clip on both sides (B = 1: the single clip): t1 below is the row
// clip * T1 + t1' of the output, and its window starts at input row clip * T + 2 t1' — inside the clip by construction.
__global__ void k_audio_conv1(const float* __restrict__ feats, const float* __restrict__ mean,
                              const float* __restrict__ istd, const uint16_t* __restrict__ w,
                              const float* __restrict__ b, float* __restrict__ out, int B, int T, int F, int C) {
    const int T1 = (T - 3) / 2 + 1, F1 = (F - 3) / 2 + 1;
    const long total = (long)B * T1 * F1 * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int f1 = (int)((i / C) % F1);
        const int row = (int)(i / ((long)C * F1));
        const int clip = row / T1, t1 = row - clip * T1;
        const float* __restrict__ fc = feats + (long)clip * T * F;
        float acc = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int f = 2 * f1 + kw;
                const float xv = (fc[(long)(2 * t1 + kh) * F + f] - mean[f]) * istd[f];
                acc = fmaf(bf16_to_f32(w[c * 9 + kh * 3 + kw]), xv, acc);
            }
        out[i] = fmaxf(acc + b[c], 0.f);
    }
}

// ---- Whale tail of a padded batch: masked_fill_(~mask_pad, 0) into a layout with `gap` zero rows behind every clip ----
// y[b][s][:] = s < klens[b] ? x[b][s][:] : 0 for s in [0, S + gap)   (init_model.py:121-127; the gap is the adapter's right padding)
__global__ void k_audio_mask_rows(const float* __restrict__ x, long ldx, float* __restrict__ y, long ldy,
                                  const int* __restrict__ klens, int B, int S, int gap, int cols4) {
    const int So = S + gap;
    const long total = (long)B * So * cols4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % cols4);
        const long row = i / cols4;
        const int b = (int)(row / So), s = (int)(row - (long)b * So);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s < S && s < klens[b]) v = *reinterpret_cast<const float4*>(x + ((long)b * S + s) * ldx + 4 * c4);
        *reinterpret_cast<float4*>(y + row * ldy + 4 * c4) = v;
    }
}

// ---- Mixtral prefill: rotate-half RoPE on q,k and KV-cache write ------------------------
// qkv rows: [q (nq*128) | k (nkv*128) | v (nkv*128)]; token s sits at position pos0+s.
// SEG: the rows belong to nseg segments of different paged sequences (VhSeg, row0 ascending): the row's segment is found by
// bisection, its position is pos0 + (row - row0) and its page table the segment's.
template <bool SEG>
__global__ void k_rope_kv(const float* __restrict__ qkv, long ldqkv, float* __restrict__ q_out,
                          float* __restrict__ kcache, float* __restrict__ vcache,
                          const float* __restrict__ rope_cos, const float* __restrict__ rope_sin, int S, int pos0,
                          int nq, int nkv, int max_ctx, const int* __restrict__ table,
                          const int* __restrict__ nslab_dev, long slab_stride, const VhSeg* __restrict__ segs, int nseg) {
    const int nh = nq + 2 * nkv;
    const long total = (long)S * nh * 64;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int d = (int)(i & 63);
        const int hh = (int)((i >> 6) % nh);
        const int s = (int)(i / ((long)nh * 64));
        int pos = pos0 + s;
        if (SEG) {
            int lo = 0, hi = nseg - 1;                     // last segment whose row0 <= s
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (segs[mid].row0 <= s) lo = mid; else hi = mid - 1;
            }
            pos = segs[lo].pos0 + (s - segs[lo].row0);
            table = segs[lo].table;
        }
        const int row = table ? table[pos >> 6] * 64 + (pos & 63) : pos;   // paged KV cache: physical row of this position
        const float* src = qkv + (size_t)s * ldqkv + hh * 128;
        float a = src[d], bq = src[d + 64];
        if (nslab_dev) {                                   // K-split projection: the partial slabs are summed here
            const int ns = *nslab_dev;
            for (int k = 1; k < ns; ++k) { a += src[(size_t)k * slab_stride + d]; bq += src[(size_t)k * slab_stride + d + 64]; }
        }
        if (hh < nq + nkv) {
            const float c = rope_cos[(size_t)pos * 64 + d], sn = rope_sin[(size_t)pos * 64 + d];
            const float ra = a * c - bq * sn, rb = bq * c + a * sn;
            float* dst = (hh < nq) ? (q_out + ((size_t)s * nq + hh) * 128)
                                   : (kcache + ((size_t)(hh - nq) * max_ctx + row) * 128);
            dst[d] = ra; dst[d + 64] = rb;
        } else {
            float* dst = vcache + ((size_t)(hh - nq - nkv) * max_ctx + row) * 128;
            dst[d] = a; dst[d + 64] = bq;
        }
    }
}

// ---- the same, tile-wise, for a ONE-SHOT prefill whose attention is the flash kernel (k_attn_fa, vh_attn.hip): besides q_out
// and the fp32 KV cache it writes K and V as the MFMA-ready bf16 hi/lo tile images that kernel keeps in LDS, converted ONCE where
// they are produced (r04-r05: every block of k_attn_fa converted every tile it read from fp32 — a third of that kernel).
// grid (64-row tiles, nkv + nq): y < nkv: K / V tile of KV head y (threads 256-511 K with RoPE, 0-255 V; the image is assembled in
// LDS with k_attn_fa's staging arithmetic and copied out in 16-byte pieces); y >= nkv: query head y - nkv.
// Image layout (64 KB per (head, tile), = the LDS buffer of k_attn_fa): K planes [half][64 keys][128 B], 16-byte chunks
// XOR-swizzled by (key >> 1) & 7; V planes TRANSPOSED [rho(col)][64 keys], rho(d) = 16 (d % 8) + d / 8, chunks swizzled by
// (rho >> 1) & 7.  Rows past S are zeros (finite: their probabilities are 0).  Same fp32 values as k_rope_kv (same slab order).
#define KVI_PL 16384
typedef __attribute__((ext_vector_type(2))) __bf16 kvi_bf16x2;
typedef __attribute__((ext_vector_type(2))) float kvi_f32x2;
__device__ __forceinline__ void kvi_split2(float a, float b, uint32_t& hi, uint32_t& lo) {
    const kvi_f32x2 v = {a, b};
    const kvi_bf16x2 h = __builtin_convertvector(v, kvi_bf16x2);
    const kvi_f32x2 r = v - __builtin_convertvector(h, kvi_f32x2);
    const kvi_bf16x2 l = __builtin_convertvector(r, kvi_bf16x2);
    hi = __builtin_bit_cast(uint32_t, h);
    lo = __builtin_bit_cast(uint32_t, l);
}
__device__ __forceinline__ f32x4 kvi_sum4(const float* src, int ns, long slab_stride) {
    f32x4 a = *reinterpret_cast<const f32x4*>(src);
    for (int k = 1; k < ns; ++k) a += *reinterpret_cast<const f32x4*>(src + (size_t)k * slab_stride);
    return a;
}
__global__ __launch_bounds__(512) void k_rope_kv_img(const float* __restrict__ qkv, long ldqkv, float* __restrict__ q_out,
                                                     float* __restrict__ kcache, float* __restrict__ vcache,
                                                     const float* __restrict__ rope_cos, const float* __restrict__ rope_sin, int S,
                                                     int nq, int nkv, int max_ctx, const int* __restrict__ table,
                                                     const int* __restrict__ nslab_dev, long slab_stride,
                                                     unsigned char* __restrict__ img, int img_tiles) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * KVI_PL];
    const int t = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const int ns = nslab_dev ? *nslab_dev : 1;
    if (y >= nkv) {                                        // ---- q rows of head y - nkv (one block per head and tile: 2 items per thread)
        const int head = y - nkv;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int item = tid + 512 * i;
            const int c = item & 15, r = item >> 4;
            const int s = 64 * t + r;
            if (s >= S) continue;
            const float* src = qkv + (size_t)s * ldqkv + head * 128;
            const f32x4 a = kvi_sum4(src + 4 * c, ns, slab_stride), b = kvi_sum4(src + 64 + 4 * c, ns, slab_stride);
            const f32x4 cs = *reinterpret_cast<const f32x4*>(rope_cos + (size_t)s * 64 + 4 * c);
            const f32x4 sn = *reinterpret_cast<const f32x4*>(rope_sin + (size_t)s * 64 + 4 * c);
            float* dst = q_out + ((size_t)s * nq + head) * 128;
            *reinterpret_cast<f32x4*>(dst + 4 * c) = a * cs - b * sn;
            *reinterpret_cast<f32x4*>(dst + 64 + 4 * c) = b * cs + a * sn;
        }
        return;
    }
    const int h = y;
    if (tid >= 256) {                                      // ---- K: RoPE, cache rows, hi/lo planes
        const int ftid = tid - 256;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int item = ftid + 256 * i;
            const int c = item & 15, key = item >> 4;
            const int s = 64 * t + key;
            const bool valid = s < S;
            const int sc = valid ? s : S - 1;
            const float* src = qkv + (size_t)sc * ldqkv + (size_t)(nq + h) * 128;
            const f32x4 a = kvi_sum4(src + 4 * c, ns, slab_stride), b = kvi_sum4(src + 64 + 4 * c, ns, slab_stride);
            const f32x4 cs = *reinterpret_cast<const f32x4*>(rope_cos + (size_t)sc * 64 + 4 * c);
            const f32x4 sn = *reinterpret_cast<const f32x4*>(rope_sin + (size_t)sc * 64 + 4 * c);
            f32x4 ra = a * cs - b * sn, rb = b * cs + a * sn;
            if (valid) {
                const int row = table ? table[s >> 6] * 64 + (s & 63) : s;
                float* kc = kcache + ((size_t)h * max_ctx + row) * 128;
                *reinterpret_cast<f32x4*>(kc + 4 * c) = ra;
                *reinterpret_cast<f32x4*>(kc + 64 + 4 * c) = rb;
            } else {
                ra = f32x4{0.f, 0.f, 0.f, 0.f};
                rb = ra;
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const f32x4 v = half ? rb : ra;
                const int fk_c = c + 16 * half;
                uint32_t h0, l0, h1, l1;
                kvi_split2(v[0], v[1], h0, l0);
                kvi_split2(v[2], v[3], h1, l1);
                const int off = (fk_c >> 4) * 8192 + key * 128 + (((((fk_c & 15) >> 1)) ^ ((key >> 1) & 7)) << 4) + (fk_c & 1) * 8;
                *reinterpret_cast<uint2*>(lds + off) = make_uint2(h0, h1);
                *reinterpret_cast<uint2*>(lds + KVI_PL + off) = make_uint2(l0, l1);
            }
        }
    } else {                                               // ---- V: cache rows, transposed hi/lo planes
        const int fv_kg = tid >> 4, fv_cg = tid & 15;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            f32x4 st[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int key = 4 * fv_kg + u;
                const int s = 64 * t + key;
                const bool valid = s < S;
                const int sc = valid ? s : S - 1;
                const int col = 4 * fv_cg + 64 * part;
                f32x4 v = kvi_sum4(qkv + (size_t)sc * ldqkv + (size_t)(nq + nkv + h) * 128 + col, ns, slab_stride);
                if (valid) {
                    const int row = table ? table[s >> 6] * 64 + (s & 63) : s;
                    *reinterpret_cast<f32x4*>(vcache + ((size_t)h * max_ctx + row) * 128 + col) = v;
                } else {
                    v = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                st[u] = v;
            }
            const int cg = fv_cg + 16 * part;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t h01, l01, h23, l23;
                kvi_split2(st[0][j], st[1][j], h01, l01);
                kvi_split2(st[2][j], st[3][j], h23, l23);
                const int d = 4 * cg + j;
                const int rho = 16 * (d % 8) + d / 8;
                const int off = rho * 128 + ((((fv_kg >> 1)) ^ ((rho >> 1) & 7)) << 4) + (fv_kg & 1) * 8;
                *reinterpret_cast<uint2*>(lds + 2 * KVI_PL + off) = make_uint2(h01, h23);
                *reinterpret_cast<uint2*>(lds + 3 * KVI_PL + off) = make_uint2(l01, l23);
            }
        }
    }
    __syncthreads();
    uint4* dst = reinterpret_cast<uint4*>(img + ((size_t)h * img_tiles + t) * (4 * KVI_PL));
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i * 512 + tid] = reinterpret_cast<const uint4*>(lds)[i * 512 + tid];
}

// ---- embedding gather + multimodal splice (vita_arch.py:237-321) ------------------------
// host builds, per destination row, kind (0 text / 1 image / 2 audio) and source index.
__global__ __launch_bounds__(256) void k_embed_splice(const int* __restrict__ kind, const int* __restrict__ idx,
                                                      const uint16_t* __restrict__ embed,
                                                      const float* __restrict__ img, const float* __restrict__ aud,
                                                      float* __restrict__ out, int S, int H) {
    const int r = blockIdx.x;
    if (r >= S) return;
    const int k = kind[r];
    const long src = idx[r];
    float* dst = out + (size_t)r * H;
    if (k == 0) {
        for (int c = threadIdx.x; c < H; c += 256) dst[c] = bf16_to_f32(embed[src * H + c]);
    } else {
        const float* sp = (k == 1 ? img : aud) + src * H;
        for (int c = threadIdx.x; c < H; c += 256) dst[c] = sp[c];
    }
}

// counting sort of the 2S (token, slot) entries by expert: wave e owns expert e.
// sorted order inside an expert is ascending entry index -> deterministic.
// The ids are staged in LDS by all waves at once (ONE memory round trip; r02 scanned global memory chunk by chunk, twice:
// 36 dependent L2 round trips = 12.6 us per layer for 1104 entries); chunks of MS_CHUNK entries for long prompts.
#define MS_CHUNK 8192
__global__ void k_moe_sort(const int* __restrict__ ids, int S, int E, int* __restrict__ group_off,
                           int* __restrict__ sorted_tok, int* __restrict__ sorted_slot) {
    __shared__ int cnt[8];
    __shared__ signed char ids_s[MS_CHUNK];
    const int lane = threadIdx.x & 63, e = threadIdx.x >> 6;
    const int n = 2 * S;
    int c = 0;
    for (int b0 = 0; b0 < n; b0 += MS_CHUNK) {
        const int nb = min(MS_CHUNK, n - b0);
        __syncthreads();
        for (int i = threadIdx.x; i < nb; i += blockDim.x) ids_s[i] = (signed char)ids[b0 + i];
        __syncthreads();
        for (int i0 = 0; i0 < nb; i0 += 64) {
            const int i = i0 + lane;
            c += __popcll(__ballot((i < nb) && (ids_s[i] == e)));
        }
    }
    if (lane == 0) cnt[e] = c;
    __syncthreads();
    int base = 0;
    for (int j = 0; j < e; ++j) base += cnt[j];
    if (lane == 0) {
        group_off[e] = base;
        if (e == E - 1) group_off[E] = base + c;
    }
    int run = base;
    for (int b0 = 0; b0 < n; b0 += MS_CHUNK) {
        const int nb = min(MS_CHUNK, n - b0);
        if (n > MS_CHUNK) {                              // (a single chunk is still resident from the counting pass)
            __syncthreads();
            for (int i = threadIdx.x; i < nb; i += blockDim.x) ids_s[i] = (signed char)ids[b0 + i];
            __syncthreads();
        }
        for (int i0 = 0; i0 < nb; i0 += 64) {
            const int i = i0 + lane;
            const bool f = (i < nb) && (ids_s[i] == e);
            const unsigned long long bal = __ballot(f);
            if (f) {
                const int p = run + __popcll(bal & ((1ull << lane) - 1ull));
                sorted_tok[p] = (b0 + i) >> 1;
                sorted_slot[p] = b0 + i;
            }
            run += __popcll(bal);
        }
    }
}

// x[s,:] += w0 * sum_ks y[ks][2s,:] + w1 * sum_ks y[ks][2s+1,:]   (MixtralExperts index_add_,
// modeling_mixtral.py:85-93; ks = the K-split slabs of the down projection, added in a fixed order)
__global__ void k_moe_combine(float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ wts,
                              int S, int H, int nslab, long slab_stride, const int* __restrict__ nslab_dev) {
    if (nslab_dev) nslab = *nslab_dev;                  // the down projection chose its K split on the device
    const long total = (long)S * (H / 4);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long s = i / (H / 4);
        const int c = (int)(i % (H / 4));
        const float w0 = wts[s * 2], w1 = wts[s * 2 + 1];
        float4 a = reinterpret_cast<float4*>(x + s * H)[c];
        float4 y0 = reinterpret_cast<const float4*>(y + (2 * s) * H)[c];
        float4 y1 = reinterpret_cast<const float4*>(y + (2 * s + 1) * H)[c];
        for (int k = 1; k < nslab; ++k) {
            const float4 p0 = reinterpret_cast<const float4*>(y + k * slab_stride + (2 * s) * H)[c];
            const float4 p1 = reinterpret_cast<const float4*>(y + k * slab_stride + (2 * s + 1) * H)[c];
            y0.x += p0.x; y0.y += p0.y; y0.z += p0.z; y0.w += p0.w;
            y1.x += p1.x; y1.y += p1.y; y1.z += p1.z; y1.w += p1.w;
        }
        a.x += w0 * y0.x + w1 * y1.x; a.y += w0 * y0.y + w1 * y1.y;
        a.z += w0 * y0.z + w1 * y1.z; a.w += w0 * y0.w + w1 * y1.w;
        reinterpret_cast<float4*>(x + s * H)[c] = a;
    }
}

// ---- synthetic weights: a counter-based generator with an exact bf16 value set --------------------------
// value(seed, i) = (sum of four 6-bit fields of splitmix64(seed + i * golden) - 126) * 2^-11: an integer in
// [-126, 126] times a power of two, i.e. exactly representable in bf16 (8 significant bits), approximately
// normal with sigma = 0.018 (N(0, 0.02) initialisation).  The SAME integer arithmetic runs in
// oracle/hashfill.c on the host, so the CPU oracle and the device hold identical weights for ANY tensor size
// without a 94 GB host copy (tests/test_realgeom_gpu.py, bench.py).  Element (r, c) of the filled view is
// sample idx0 + r * ld_src + c, so row / column slices of a logical tensor (tensor-parallel shards) get the
// values of the full tensor.
__device__ __forceinline__ uint16_t hash_bf16(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + idx * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    const int v = (int)(z & 63) + (int)((z >> 6) & 63) + (int)((z >> 12) & 63) + (int)((z >> 18) & 63) - 126;
    return (uint16_t)(__float_as_uint((float)v * 0.00048828125f) >> 16);   // exact: |v| < 2^7
}
__global__ void k_fill_hash_bf16(uint16_t* __restrict__ dst, long rows, long cols, long ld_dst, long ld_src, long idx0,
                                 uint64_t seed) {
    const long total = rows * cols;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols, c = i - r * cols;
        dst[r * ld_dst + c] = hash_bf16(seed, (uint64_t)(idx0 + r * ld_src + c));
    }
}

inline int grid_for(long total, int block) {
    long g = (total + block - 1) / block;
    if (g > 4096) g = 4096;  // grid-stride beyond ~16 blocks/CU (guide G11)
    if (g < 1) g = 1;
    return (int)g;
}

// batched decode, streaming-MoE path: residual stream of every sequence of the iteration gathered into contiguous rows.
// Slot layout (vh_api.hip): seq_x[slot] = {xa, xb, delta_attn, delta_moe}[H]; x = xb + delta_attn is also stored to xa,
// exactly what k_dec_gateup's prologue leaves there.
__global__ __launch_bounds__(256) void k_gather_rows(float* __restrict__ seq_x, const int* __restrict__ slots, int H,
                                                     float* __restrict__ rows) {
    const int b = blockIdx.x;
    float* x = seq_x + (size_t)slots[b] * 4 * H;
    const f32x4* xb = reinterpret_cast<const f32x4*>(x + H);
    const f32x4* da = reinterpret_cast<const f32x4*>(x + 2 * H);
    f32x4* xa = reinterpret_cast<f32x4*>(x);
    f32x4* out = reinterpret_cast<f32x4*>(rows + (size_t)b * H);
    for (int c = threadIdx.x; c < H / 4; c += 256) {
        const f32x4 v = xb[c] + da[c];
        xa[c] = v;
        out[c] = v;
    }
}
// ---- int8 expert weights: per-row absmax quantisation --------------------------------------------------------
// s[r] = max_k |w[r,k]| / 127, q = clamp(rint(w / s), -127, 127) (0 for an all-zero row), both divisions IEEE (the numpy
// restatement in tests/q8_ref.py is matched bit for bit).  The scale is taken over all `cols`; only the columns
// [col0, col0 + ncols) are written (a tensor-parallel rank's slice of w2 with the full-row scale).  One block per row.
__global__ __launch_bounds__(256) void k_quant_rows_i8(const uint16_t* __restrict__ w, int cols, long ld_src, int col0, int ncols,
                                                       int8_t* __restrict__ q, long ld_dst, float* __restrict__ s) {
    __shared__ float red[8];
    const long r = blockIdx.x;
    const uint16_t* row = w + r * ld_src;
    float mx = 0.f;
    for (int k = threadIdx.x; k < cols; k += 256) mx = fmaxf(mx, fabsf(bf16_to_f32(row[k])));
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float sc = __fdiv_rn(mx, 127.0f);
    if (threadIdx.x == 0) s[r] = sc;
    int8_t* out = q + r * ld_dst;
    for (int k = threadIdx.x; k < ncols; k += 256) {
        float v = 0.f;
        if (sc != 0.f) v = fminf(fmaxf(rintf(__fdiv_rn(bf16_to_f32(row[col0 + k]), sc)), -127.f), 127.f);
        out[k] = (int8_t)(int)v;
    }
}

// ---- MXFP4 expert weights: e2m1 codes with one E8M0 scale byte per 32 consecutive elements of a row ------------
// amax over the block, se = max(floor(log2 amax) - 2, -125) from the exponent field (0 for a zero block), byte = se + 127,
// v = |w| 2^-se (exact) saturated at 6 and rounded to the nearest e2m1 magnitude, ties to the even code; the sign bit only with
// a non-zero magnitude (tests/q4_ref.py is matched bit for bit).  A thread takes 8 elements (16 bytes in, 4 bytes out), the four
// lanes of a block share the amax; only the columns [col0, col0 + ncols) are read and written.
__global__ __launch_bounds__(256) void k_quant_mxfp4(const uint16_t* __restrict__ w, long ld_src, int col0, int pieces, long total,
                                                     uint8_t* __restrict__ codes, long ld_codes, uint8_t* __restrict__ scales,
                                                     long ld_scales) {
    // grid-stride; total % 4 == 0 and the stride is a multiple of 256: the four lanes of a block stay together
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / pieces;
        const int p = (int)(idx - r * pieces);
        const uint4 raw = *reinterpret_cast<const uint4*>(w + r * ld_src + col0 + p * 8);
        const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
        float v[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(wd[i] << 16);
            v[2 * i + 1] = __uint_as_float(wd[i] & 0xffff0000u);
        }
        float mx = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fabsf(v[i]));
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        const int ef = (int)((__float_as_uint(mx) >> 23) & 0xffu);
        int se = ef - 127 - 2;
        if (se < -125) se = -125;                      // (a bf16 denormal amax included: its floor(log2) is below -126)
        if (mx == 0.f) se = 0;
        const float inv = __uint_as_float((uint32_t)(127 - se) << 23);   // 2^-se, a normal number for se in [-125, 125]
        uint32_t out = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float a = fminf(fabsf(v[i]) * inv, 6.0f);
            const uint32_t m = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
            const uint32_t sg = (v[i] < 0.f && m != 0) ? 8u : 0u;
            out |= (sg | m) << (4 * i);
        }
        *reinterpret_cast<uint32_t*>(codes + r * ld_codes + p * 4) = out;
        if ((p & 3) == 0) scales[r * ld_scales + (p >> 2)] = (uint8_t)(se + 127);
    }
}

}  // namespace

int vhk_layernorm(hipStream_t st, const float* x, long ldx, float* y, long ldy, const float* w, const float* b,
                  int rows, int cols, float eps, int act, float post_scale) {
    if (cols % 4 != 0 || cols > LN_MAXV * 256) return -1;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(k_norm_rows<false>, dim3((rows + 3) / 4), dim3(256), 0, st, x, ldx, y, ldy, w, b, rows, cols,
                       eps, act, post_scale);
    return 0;
}
int vhk_rmsnorm(hipStream_t st, const float* x, float* y, const float* w, int rows, int cols, float eps) {
    if (cols % 4 != 0 || cols > LN_MAXV * 256) return -1;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(k_norm_rows<true>, dim3((rows + 3) / 4), dim3(256), 0, st, x, (long)cols, y, (long)cols, w,
                       (const float*)nullptr, rows, cols, eps, VH_ACT_NONE, 1.0f);
    return 0;
}
int vhk_add(hipStream_t st, float* x, const float* y, long n) {
    if (n % 4 != 0) return -1;
    hipLaunchKernelGGL(k_add, dim3(grid_for(n / 4, 256)), dim3(256), 0, st, x, y, n / 4);
    return 0;
}
int vhk_add_halves(hipStream_t st, float* x, const float* a, const float* b, int rows, int cols) {
    if (cols % 8 != 0) return -1;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(k_add_halves, dim3(grid_for((long)rows * (cols / 4), 256)), dim3(256), 0, st, x, a, b, rows, cols / 4);
    return 0;
}
int vhk_hash_row_blocks(hipStream_t st, const float* x, long ldx, int rows, int cols, uint32_t* out) {
    // word positions are 32-bit: 4 * (64 * cols) + 3 must not wrap
    if (rows < 0 || cols < 1 || cols > (1 << 23) || ldx < cols) return -1;
    const int nblk = rows / 64;
    if (nblk == 0) return 0;
    if (hipMemsetAsync(out, 0, (size_t)nblk * 4 * sizeof(uint32_t), st) != hipSuccess) return -3;
    const bool vec = (cols % 4) == 0 && (ldx % 4) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const dim3 grid(64 / HASH_ROWS_PER_WG, nblk);
    if (vec) hipLaunchKernelGGL(k_hash_row_blocks<true>, grid, dim3(256), 0, st, x, ldx, cols, out);
    else hipLaunchKernelGGL(k_hash_row_blocks<false>, grid, dim3(256), 0, st, x, ldx, cols, out);
    hipLaunchKernelGGL(k_hash_finish, dim3((nblk * 4 + 255) / 256), dim3(256), 0, st, out, nblk * 4);
    return 0;
}
int vhk_quant_rows_i8(hipStream_t st, const uint16_t* w, long rows, int cols, long ld_src, int col0, int ncols, int8_t* q,
                      long ld_dst, float* s) {
    if (rows < 0 || rows > 0x7fffffffL || cols < 1 || ld_src < cols || col0 < 0 || ncols < 1 || col0 + ncols > cols || ld_dst < ncols)
        return -1;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(k_quant_rows_i8, dim3((unsigned)rows), dim3(256), 0, st, w, cols, ld_src, col0, ncols, q, ld_dst, s);
    return 0;
}
int vhk_quant_mxfp4(hipStream_t st, const uint16_t* w, long rows, int cols, long ld_src, int col0, int ncols, uint8_t* codes,
                    long ld_codes, uint8_t* scales, long ld_scales) {
    if (rows < 0 || rows > 0x7fffffffL || cols < 1 || ld_src < cols || (ld_src % 8) != 0 || col0 < 0 || ncols < 1 || col0 + ncols > cols ||
        (col0 % 32) != 0 || (ncols % 32) != 0 || ld_codes < ncols / 2 || (ld_codes % 4) != 0 || ld_scales < ncols / 32 ||
        (reinterpret_cast<uintptr_t>(w) & 15) != 0 || (reinterpret_cast<uintptr_t>(codes) & 3) != 0)
        return -1;
    if (rows == 0) return 0;
    const int pieces = ncols / 8;
    const long total = rows * pieces;
    hipLaunchKernelGGL(k_quant_mxfp4, dim3(grid_for(total, 256)), dim3(256), 0, st, w, ld_src, col0, pieces, total, codes, ld_codes,
                       scales, ld_scales);
    return 0;
}
int vhk_cast_bf16_f32(hipStream_t st, const uint16_t* in, float* out, long n) {
    hipLaunchKernelGGL(k_cast_bf16_f32, dim3(grid_for(n, 256)), dim3(256), 0, st, in, out, n);
    return 0;
}
int vhk_vit_patchify(hipStream_t st, const float* pix, float* out, int n, int img, int patch, int kpad) {
    if (img % patch != 0 || kpad < 3 * patch * patch) return -1;
    const int g = img / patch;
    hipLaunchKernelGGL(k_vit_patchify, dim3(grid_for((long)n * g * g * kpad, 256)), dim3(256), 0, st, pix, out, n, img,
                       patch, kpad);
    return 0;
}
int vhk_vit_assemble(hipStream_t st, const float* patches, const uint16_t* cls, const uint16_t* pos, float* x, int n,
                     int ntok, int hid) {
    hipLaunchKernelGGL(k_vit_assemble, dim3(grid_for((long)n * ntok * hid, 256)), dim3(256), 0, st, patches, cls, pos,
                       x, n, ntok, hid);
    return 0;
}
int vhk_vit_pixel_shuffle(hipStream_t st, const float* x, float* out, int n, int grid, int hid, float mul) {
    if (grid % 2 != 0) return -1;
    hipLaunchKernelGGL(k_vit_pixel_shuffle, dim3(grid_for((long)n * (grid / 2) * (grid / 2) * 4 * hid, 256)),
                       dim3(256), 0, st, x, out, n, grid, hid, mul);
    return 0;
}
int vhk_audio_conv1(hipStream_t st, const float* feats, const float* mean, const float* istd, const uint16_t* w,
                    const float* b, float* out, int B, int T, int F, int C) {
    if (B < 1 || T < 3 || F < 3) return -1;
    const long total = (long)B * ((T - 3) / 2 + 1) * ((F - 3) / 2 + 1) * C;
    if ((long)B * ((T - 3) / 2 + 1) >= (1L << 31)) return -1;
    hipLaunchKernelGGL(k_audio_conv1, dim3(grid_for(total, 256)), dim3(256), 0, st, feats, mean, istd, w, b, out, B, T, F,
                       C);
    return 0;
}
int vhk_audio_mask_rows(hipStream_t st, const float* x, long ldx, float* y, long ldy, const int* klens, int B, int S, int gap,
                        int cols) {
    if (B < 1 || S < 1 || gap < 0 || cols < 4 || (cols % 4) != 0 || (ldx % 4) != 0 || (ldy % 4) != 0 || ldx < cols || ldy < cols) return -1;
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(y) & 15)) return -1;
    const long total = (long)B * (S + gap) * (cols / 4);
    hipLaunchKernelGGL(k_audio_mask_rows, dim3(grid_for(total, 256)), dim3(256), 0, st, x, ldx, y, ldy, klens, B, S, gap, cols / 4);
    return 0;
}
int vhk_rope_kv(hipStream_t st, const float* qkv, long ldqkv, float* q_out, float* kcache, float* vcache,
                const float* rope_cos, const float* rope_sin, int S, int pos0, int nq, int nkv, int max_ctx,
                const int* table, const int* nslab_dev, long slab_stride) {
    if (S == 0) return 0;
    hipLaunchKernelGGL(k_rope_kv<false>, dim3(grid_for((long)S * (nq + 2 * nkv) * 64, 256)), dim3(256), 0, st, qkv, ldqkv,
                       q_out, kcache, vcache, rope_cos, rope_sin, S, pos0, nq, nkv, max_ctx, table, nslab_dev, slab_stride,
                       (const VhSeg*)nullptr, 0);
    return 0;
}
int vhk_rope_kv_segs(hipStream_t st, const float* qkv, long ldqkv, float* q_out, float* kcache, float* vcache,
                     const float* rope_cos, const float* rope_sin, int S, const VhSeg* segs, int nseg, int nq, int nkv,
                     int max_ctx, const int* nslab_dev, long slab_stride) {
    if (S == 0) return 0;
    if (!segs || nseg < 1) return -1;
    hipLaunchKernelGGL(k_rope_kv<true>, dim3(grid_for((long)S * (nq + 2 * nkv) * 64, 256)), dim3(256), 0, st, qkv, ldqkv,
                       q_out, kcache, vcache, rope_cos, rope_sin, S, 0, nq, nkv, max_ctx, (const int*)nullptr, nslab_dev,
                       slab_stride, segs, nseg);
    return 0;
}
int vhk_rope_kv_img(hipStream_t st, const float* qkv, long ldqkv, float* q_out, float* kcache, float* vcache,
                    const float* rope_cos, const float* rope_sin, int S, int nq, int nkv, int max_ctx,
                    const int* table, const int* nslab_dev, long slab_stride, unsigned char* img, int img_tiles) {
    if (S == 0) return 0;
    const int tiles = (S + 63) / 64;
    if (nq != 4 * nkv || !img || tiles > img_tiles || (ldqkv % 4) != 0 || (slab_stride % 4) != 0) return -1;
    hipLaunchKernelGGL(k_rope_kv_img, dim3(tiles, nkv + nq), dim3(512), 0, st, qkv, ldqkv, q_out, kcache, vcache, rope_cos, rope_sin, S,
                       nq, nkv, max_ctx, table, nslab_dev, slab_stride, img, img_tiles);
    return 0;
}
int vhk_embed_splice(hipStream_t st, const int* src_kind, const int* src_idx, const uint16_t* embed,
                     const float* img_feats, const float* aud_feats, float* out, int S, int H) {
    if (S == 0) return 0;
    hipLaunchKernelGGL(k_embed_splice, dim3(S), dim3(256), 0, st, src_kind, src_idx, embed, img_feats, aud_feats, out,
                       S, H);
    return 0;
}
int vhk_rmsnorm_route(hipStream_t st, float* x, float* y, uint16_t* y_hi, uint16_t* y_lo, const float* w, int rows,
                      int cols, float eps, const uint16_t* Wg, int E, int* ids, float* wts, const VhRowUpdate* upd) {
    if (cols % 4 != 0 || cols > RR_MAXJ * 1024 || E == 1 || E < 0 || E > 8 || (y_hi && !y_lo) || (!y && !y_hi)) return -1;   // E = 0: norm only
    if (E > 0 && (!Wg || !ids || !wts)) return -1;
    if (upd && (!upd->src || (upd->ld % 4) != 0 || (upd->stride % 4) != 0 || (!upd->nslab_dev && upd->nslab < 1))) return -1;
    if (upd && upd->wts && upd->wts == wts && E > 0) return -1;   // the routing weights being applied must not be the ones being written
    if (rows == 0) return 0;
    const VhRowUpdate u = upd ? *upd : VhRowUpdate{};
    if (!upd)
        hipLaunchKernelGGL(k_rmsnorm_route<0>, dim3(rows), dim3(256), 0, st, x, y, y_hi, y_lo, w, rows, cols, eps, Wg, E, ids, wts, u);
    else if (!u.wts)
        hipLaunchKernelGGL(k_rmsnorm_route<1>, dim3(rows), dim3(256), 0, st, x, y, y_hi, y_lo, w, rows, cols, eps, Wg, E, ids, wts, u);
    else
        hipLaunchKernelGGL(k_rmsnorm_route<2>, dim3(rows), dim3(256), 0, st, x, y, y_hi, y_lo, w, rows, cols, eps, Wg, E, ids, wts, u);
    return 0;
}
// ---- the router alone (per-operator entry vh_router_top2; HF MixtralSparseMoeBlock: gate -> fp32 softmax -> top-2 ->
// renormalise, modeling_mixtral.py:96-111 / vllm_file/mixtral.py:398-411): one wave per token, fp32 throughout ----------
__global__ __launch_bounds__(256) void k_router_top2(const float* __restrict__ x, long ldx, const uint16_t* __restrict__ Wg, int E,
                                                     int H, int rows, int* __restrict__ ids, float* __restrict__ wts,
                                                     float* __restrict__ probs) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float lg[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) lg[e] = 0.f;
    for (int c = lane; c * 8 < H; c += 64) {
        const float4 a = reinterpret_cast<const float4*>(x + (size_t)row * ldx)[c * 2];
        const float4 b = reinterpret_cast<const float4*>(x + (size_t)row * ldx)[c * 2 + 1];
        const float xv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < E) lg[e] += dot8_bf16_f32(reinterpret_cast<const uint4*>(Wg + (size_t)e * H)[c], xv);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) lg[e] = wave_sum(lg[e]);
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; ++e) if (e < E) mx = fmaxf(mx, lg[e]);
    float pr[8], sum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { pr[e] = e < E ? expf(lg[e] - mx) : 0.f; sum += pr[e]; }
    int e0 = 0, e1 = 0;
    float b0 = -1.f, b1 = -1.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { pr[e] /= sum; if (e < E && pr[e] > b0) { b0 = pr[e]; e0 = e; } }
#pragma unroll
    for (int e = 0; e < 8; ++e) if (e < E && e != e0 && pr[e] > b1) { b1 = pr[e]; e1 = e; }
    if (lane == 0) {
        ids[2 * row] = e0; ids[2 * row + 1] = e1;
        wts[2 * row] = b0 / (b0 + b1); wts[2 * row + 1] = b1 / (b0 + b1);
        if (probs)
            for (int e = 0; e < E; ++e) probs[(size_t)row * E + e] = pr[e];
    }
}

int vhk_router_top2(hipStream_t st, const float* x, long ldx, const uint16_t* Wg, int E, int H, int rows, int* ids, float* wts,
                    float* probs) {
    if (E < 2 || E > 8 || H % 8 != 0 || (ldx % 4) != 0 || rows < 0) return -1;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(k_router_top2, dim3((rows + 3) / 4), dim3(256), 0, st, x, ldx, Wg, E, H, rows, ids, wts, probs);
    return 0;
}

int vhk_moe_sort(hipStream_t st, const int* ids, int S, int E, int* group_off, int* sorted_tok, int* sorted_slot) {
    if (E > 8) return -1;
    hipLaunchKernelGGL(k_moe_sort, dim3(1), dim3(64 * E), 0, st, ids, S, E, group_off, sorted_tok, sorted_slot);
    return 0;
}
int vhk_moe_combine(hipStream_t st, float* x, const float* y, const float* wts, int S, int H, int nslab,
                    long slab_stride, const int* nslab_dev) {
    if (H % 4 != 0 || nslab < 1 || (slab_stride % 4) != 0) return -1;
    if (S == 0) return 0;
    hipLaunchKernelGGL(k_moe_combine, dim3(grid_for((long)S * (H / 4), 256)), dim3(256), 0, st, x, y, wts, S, H, nslab,
                       slab_stride, nslab_dev);
    return 0;
}
int vhk_gather_rows(hipStream_t st, float* seq_x, const int* slots, int n, int H, float* rows) {
    if (n < 1 || (H % 4) != 0) return -1;
    hipLaunchKernelGGL(k_gather_rows, dim3(n), dim3(256), 0, st, seq_x, slots, H, rows);
    return 0;
}
int vhk_sum_slabs(hipStream_t st, float* dst, long ldd, const float* src, long lds, int rows, int cols,
                  const int* nslab_dev, int nslab, long stride, int accumulate) {
    if ((cols % 4) || (ldd % 4) || (lds % 4) || (stride % 4) || rows < 0) return -1;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(k_sum_slabs, dim3(grid_for((long)rows * (cols / 4), 256)), dim3(256), 0, st, dst, ldd, src, lds, rows,
                       cols / 4, nslab_dev, nslab, stride, accumulate);
    return 0;
}
int vhk_fill_hash_bf16(hipStream_t st, uint16_t* dst, long rows, long cols, long ld_dst, long ld_src, long idx0,
                       uint64_t seed) {
    if (rows < 0 || cols < 0 || ld_dst < cols) return -1;
    if (rows == 0 || cols == 0) return 0;
    hipLaunchKernelGGL(k_fill_hash_bf16, dim3(grid_for(rows * cols, 256)), dim3(256), 0, st, dst, rows, cols, ld_dst, ld_src,
                       idx0, seed);
    return 0;
}
