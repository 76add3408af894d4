// vh_sample.h — seeded temperature / top-k / top-p sampling on the device (included by vh_decode.hip).
//
// Gumbel-max: argmax_i (z_i + G_i), z = logit / T, G_i i.i.d. Gumbel(0, 1), is an exact draw from softmax(z).  The noise is a
// pure function of (seed, draw index, vocab index) — Philox4x64-10 (Salmon et al., SC'11) with key (seed, 0) and counter
// (i >> 2, draw, 0, 0), output word i & 3 — so a token does not depend on the grid, the TP degree, the batch-mates or the
// lookahead window that produced it; candidates leave a block as exact keys of their double scores (vhs_key3).  The whole contract (INTEGRATION.md "Sampling") is restated in numpy by tests/sampling_ref.py.
//
//   T = 0            greedy: the plain argmax (the engine keeps its greedy kernels untouched)
//   top-k            keep i iff z_i >= z_(k) (ties at the boundary kept, as HF TopKLogitsWarper)
//   top-p            on the softmax of the top-k-kept set: keep i iff the mass of kept values STRICTLY above z_i is < top_p
//                    (the maximum always, tied values together); masses exp(z - z_max) in double
//   NaN logits rank as -inf; nothing finite kept -> index sentinel (k_dec_select / vh_sample_rows map it to 0)
//
// The filter is a radix select over the order-preserving uint32 key of the fp32 logits (z is monotone in the logit, and distinct
// floats stay distinct after the double division): 4 passes of a 256-bucket histogram for the k-th value (counts), 4 more for the
// top-p cut (counts + double masses, one private histogram per wave summed in wave order, so the sums do not depend on timing),
// then one Gumbel-max pass over the kept entries.  One workgroup per row; the row is re-read from L2 by each pass.
#pragma once
#include <stdint.h>
#include "vh_kernels.h"   // VhSampleParams

#define VHS_M0 0xD2E7470EE14C6C93ull
#define VHS_M1 0xCA5A826395121157ull
#define VHS_W0 0x9E3779B97F4A7C15ull
#define VHS_W1 0xBB67AE8584CAA73Bull

// Philox4x64-10 of counter (c0, c1, 0, 0) under key (k0, k1) (Random123 philox4x64_R(10, ...))
__device__ __forceinline__ void vhs_philox(unsigned long long c0, unsigned long long c1, unsigned long long k0, unsigned long long k1,
                                           unsigned long long (&x)[4]) {
    x[0] = c0; x[1] = c1; x[2] = 0; x[3] = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += VHS_W0; k1 += VHS_W1; }
        const unsigned long long lo0 = VHS_M0 * x[0], hi0 = __umul64hi(VHS_M0, x[0]);
        const unsigned long long lo1 = VHS_M1 * x[2], hi1 = __umul64hi(VHS_M1, x[2]);
        x[0] = hi1 ^ x[1] ^ k0; x[1] = lo1; x[2] = hi0 ^ x[3] ^ k1; x[3] = lo0;
    }
}
// u = ((x >> 11) + 1/2) 2^-53 in (0, 1);  G = -log(-log(u))
__device__ __forceinline__ double vhs_gumbel_of(unsigned long long x) {
    const double u = ((double)(x >> 11) + 0.5) * 0x1p-53;
    return -log(-log(u));
}
__device__ __forceinline__ unsigned long long vhs_word(const unsigned long long (&x)[4], int j) {
    return (j & 2) ? ((j & 1) ? x[3] : x[2]) : ((j & 1) ? x[1] : x[0]);
}
// NaN -> -inf, -0 -> +0 (so that equal values have equal keys)
__device__ __forceinline__ float vhs_canon(float v) { return (v != v) ? -INFINITY : (v == 0.f ? 0.f : v); }
__device__ __forceinline__ unsigned vhs_key(float v) {
    const unsigned b = __float_as_uint(vhs_canon(v));
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float vhs_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// ---- logit rules (include/vita_hip.h vh_logit_rules; restated in numpy by tests/logit_rules_ref.py) -----------------------------
// seen word of an id: bit 31 = in the prompt, low bits = times it occurs in the output so far.  Every step is ONE IEEE fp32
// operation (no contraction): repetition (HF RepetitionPenaltyLogitsProcessor), then frequency, then presence (vLLM apply_penalties).
__device__ __forceinline__ float vhs_penalise(float x, unsigned s, float r, float f, float p) {
    // plain operators under contract(off): the product and the difference below must stay two roundings.  (__fmul_rn / __fsub_rn are
    // inline functions of the HIP headers built under the translation unit's default contraction, and the compiler fused their
    // product and difference into one fma; the division is the correctly rounded one, hipcc's default.)
#pragma clang fp contract(off)
    const unsigned c = s & 0x7fffffffu;
    if (s) x = x > 0.f ? x / r : x * r;
    const float fc = f * (float)c;
    x = x - fc;
    if (c) x = x - p;
    return x;
}
// row[i] as selection sees it: penalised when the request has a table (PEN instantiations only; the others are the plain load)
template <bool PEN>
__device__ __forceinline__ float vhs_ld(const float* __restrict__ row, int i, const VhPenalty& pen) {
    const float v = row[i];
    if (PEN) return pen.seen ? vhs_penalise(v, pen.seen[i], pen.r, pen.f, pen.p) : v;
    return v;
}
// z_i + G_i of vocab index i (temperature-only path of the LM head kernels)
__device__ __forceinline__ double vhs_perturbed(float v, int i, const VhSampleParams& p, unsigned long long draw) {
    unsigned long long x[4];
    vhs_philox((unsigned long long)(i >> 2), draw, p.seed, 0ull, x);
    return (double)vhs_canon(v) / p.T + vhs_gumbel_of(vhs_word(x, i & 3));
}

// A sampled candidate crosses blocks and ranks as the order-preserving 64-bit key of its double score, cut into three integer-valued
// floats (22 + 21 + 21 bits: exact in fp32 and in an all-reduce(sum) with zeros) at out[0], out[stride], out[2 stride]: the
// candidates then compare exactly as their double scores do, independent of the grid and of the vocab shards.
__device__ __forceinline__ void vhs_key3(double d, float* out, int stride) {
    unsigned long long u = (unsigned long long)__double_as_longlong(d);
    u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    out[0] = (float)(unsigned)(u >> 42);
    out[stride] = (float)(unsigned)((u >> 21) & 0x1FFFFFull);
    out[2 * stride] = (float)(unsigned)(u & 0x1FFFFFull);
}
__device__ __forceinline__ double vhs_unkey3(const float* in, int stride) {
    unsigned long long u = ((unsigned long long)(unsigned)in[0] << 42) | ((unsigned long long)(unsigned)in[stride] << 21) |
                           (unsigned long long)(unsigned)in[2 * stride];
    u = (u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u;
    return __longlong_as_double((long long)u);
}

template <int NW>
struct VhsShared {
    unsigned cnt[256];
    double mass[NW][256];
    double msum[256];
    double bv[NW];
    int bi[NW];
    unsigned kmax, sel_prefix;
    int sel_need;
    double sel_a, sel_target;
};

template <typename T>
__device__ __forceinline__ T vhs_wave_incl_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// key of the k-th largest value of row[0, V) (1 <= k <= V)
template <int NT, bool PEN = false>
__device__ unsigned vhs_select_count(const float* __restrict__ row, int V, int k, VhsShared<NT / 64>& sh, const VhPenalty& pen = VhPenalty{}) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned prefix = 0;
    int need = k;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned hmask = pass ? ~0u << (32 - 8 * pass) : 0u;
        for (int b = tid; b < 256; b += NT) sh.cnt[b] = 0;
        __syncthreads();
        for (int i = tid; i < V; i += NT) {
            const unsigned key = vhs_key(vhs_ld<PEN>(row, i, pen));
            if ((key & hmask) == prefix) atomicAdd(&sh.cnt[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {            // lane l owns buckets 255 - 4l .. 252 - 4l (descending values)
            int c[4], s = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = (int)sh.cnt[255 - 4 * lane - j]; s += c[j]; }
            const int incl = vhs_wave_incl_scan(s);
            const unsigned long long hit = __ballot(incl >= need);   // never empty: the range holds >= need values
            if (lane == __ffsll((long long)hit) - 1) {
                int acc = incl - s, b = 255 - 4 * lane;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (acc + c[j] >= need) { b = 255 - 4 * lane - j; break; }
                    acc += c[j];
                }
                sh.sel_prefix = prefix | ((unsigned)b << shift);
                sh.sel_need = need - acc;
            }
        }
        __syncthreads();
        prefix = sh.sel_prefix; need = sh.sel_need;
    }
    return prefix;
}

// smallest kept key of the top-p cut among keys >= lo (lo: the top-k threshold, 0 = none)
template <int NT, bool PEN = false>
__device__ unsigned vhs_select_mass(const float* __restrict__ row, int V, const VhSampleParams& p, unsigned lo, VhsShared<NT / 64>& sh,
                                    const VhPenalty& pen = VhPenalty{}) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) sh.kmax = 0;
    __syncthreads();
    unsigned km = 0;
    for (int i = tid; i < V; i += NT) km = max(km, vhs_key(vhs_ld<PEN>(row, i, pen)));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) km = max(km, (unsigned)__shfl_xor((int)km, o, 64));
    if (lane == 0) atomicMax(&sh.kmax, km);
    __syncthreads();
    const unsigned kmax = sh.kmax;
    const double zmax = (double)vhs_unkey(kmax) / p.T;
    if (!(zmax > -INFINITY)) return lo;              // nothing finite: no mass to cut
    if (!(zmax < INFINITY)) return kmax;             // +inf logits (or z overflow) hold all the mass
    unsigned prefix = 0;
    double a = 0.0, target = 0.0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned hmask = pass ? ~0u << (32 - 8 * pass) : 0u;
        for (int b = tid; b < 256; b += NT) sh.cnt[b] = 0;
        for (int b = tid; b < NW * 256; b += NT) sh.mass[b >> 8][b & 255] = 0.0;
        __syncthreads();
        for (int i = tid; i < V; i += NT) {
            const unsigned key = vhs_key(vhs_ld<PEN>(row, i, pen));
            if (key >= lo && (key & hmask) == prefix) {
                const unsigned b = (key >> shift) & 255u;
                atomicAdd(&sh.cnt[b], 1u);
                atomicAdd(&sh.mass[w][b], exp((double)vhs_unkey(key) / p.T - zmax));
            }
        }
        __syncthreads();
        for (int b = tid; b < 256; b += NT) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < NW; ++q) s += sh.mass[q][b];     // wave order: the same sum every run
            sh.msum[b] = s;
        }
        __syncthreads();
        if (tid < 64) {
            double m[4], s = 0.0;
            int c[4], cs = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { m[j] = sh.msum[255 - 4 * lane - j]; c[j] = (int)sh.cnt[255 - 4 * lane - j]; s += m[j]; cs += c[j]; }
            const double incl = vhs_wave_incl_scan(s);
            const double excl = lane ? __shfl_up(incl, 1, 64) : 0.0;
            if (pass == 0) target = p.top_p * __shfl(incl, 63, 64);      // top_p x (mass of the top-k-kept set)
            const unsigned long long hit = __ballot(a + incl >= target);
            // the first bucket whose inclusive mass reaches the target holds the cut; none (rounding): the lowest non-empty one
            const int L = hit ? __ffsll((long long)hit) - 1 : 63 - __clzll((long long)__ballot(cs > 0));
            if (lane == L) {
                double acc = a + excl, acc_last = acc;
                int b = -1, last = 255 - 4 * lane;
                for (int j = 0; j < 4; ++j) {
                    const int bk = 255 - 4 * lane - j;
                    if (c[j] > 0) {
                        if (acc + m[j] >= target) { b = bk; break; }
                        last = bk; acc_last = acc;
                    }
                    acc += m[j];
                }
                if (b < 0) { b = last; acc = acc_last; }   // no crossing (rounding): the lane's last non-empty bucket
                sh.sel_prefix = prefix | ((unsigned)b << shift);
                sh.sel_a = acc;
                sh.sel_target = target;
            }
        }
        __syncthreads();
        prefix = sh.sel_prefix; a = sh.sel_a; target = sh.sel_target;
    }
    return prefix;
}

// One row: filter (top-k, top-p) and Gumbel-max draw `draw` (T = 0: plain argmax).  Block-collective; every thread returns the
// winner (value = z + G of it, index; index 0x7fffffff when nothing finite was kept).
template <int NT, bool PEN = false>
__device__ void vhs_row(const float* __restrict__ row, int V, const VhSampleParams& p, unsigned long long draw, VhsShared<NT / 64>& sh,
                        double& best_out, int& idx_out, const VhPenalty& pen = VhPenalty{}) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool greedy = !(p.T > 0.0);
    unsigned thr = 0;
    if (!greedy && p.top_k > 0 && p.top_k < V) thr = vhs_select_count<NT, PEN>(row, V, p.top_k, sh, pen);
    if (!greedy && p.top_p < 1.0) thr = max(thr, vhs_select_mass<NT, PEN>(row, V, p, thr, sh, pen));
    double best = -INFINITY;
    int bi = 0x7fffffff;
    for (int g = tid; 4 * g < V; g += NT) {        // ascending indices per thread: the first maximum wins
        float v[4];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = 4 * g + j < V ? vhs_canon(vhs_ld<PEN>(row, 4 * g + j, pen)) : -INFINITY;
            any = any || (4 * g + j < V && vhs_key(v[j]) >= thr);
        }
        if (!any) continue;
        unsigned long long x[4] = {0, 0, 0, 0};
        if (!greedy) vhs_philox((unsigned long long)g, draw, p.seed, 0ull, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * g + j >= V || vhs_key(v[j]) < thr) continue;
            const double s = greedy ? (double)v[j] : (double)v[j] / p.T + vhs_gumbel_of(x[j]);
            if (s > best) { best = s; bi = 4 * g + j; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { sh.bv[w] = best; sh.bi[w] = bi; }
    __syncthreads();
    best = sh.bv[0]; bi = sh.bi[0];
#pragma unroll
    for (int q = 1; q < NT / 64; ++q)
        if (sh.bv[q] > best || (sh.bv[q] == best && sh.bi[q] < bi)) { best = sh.bv[q]; bi = sh.bi[q]; }
    __syncthreads();          // sh is reused by the caller's next row
    best_out = best; idx_out = bi;
}

// ---- log-probabilities of one RAW row (vLLM's raw_logprobs / HF output_logits view): lp(x) = x - (M + log sum_j exp(x_j - M)) in
// double, M the row maximum, rounded to fp32 once.  The sum is one partial per wave (each thread adds its strided elements in
// ascending order, the wave folds them in a fixed butterfly) added in wave order, so it does not depend on timing.  NaN ranks as
// -inf; a row with nothing finite gives -inf everywhere.  The top K in (logit descending, id ascending) order come from K rounds
// of a block-wide maximum over 64-bit (value key, ~id) keys: every thread keeps its best candidate below the previous winner and
// only the winner's owner looks through its elements again.  EL > 0 (V <= NT * EL): a thread's elements stay in EL registers for
// those rounds, so a round costs a wave reduction, two barriers and one wave's pass over its registers; EL = 0: the owner re-reads
// its elements from the row.  Entries past V: id -1, -inf.
template <int NW>
struct VhsLpShared {
    double part[NW];
    unsigned long long top[NW];
    unsigned kmax;
};
__device__ __forceinline__ unsigned long long vhs_lp_key(float v, int i) {
    return ((unsigned long long)vhs_key(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
}
template <int NT, int EL>
__device__ void vhs_logprobs_row(const float* __restrict__ row, int V, int tok, int K, float* __restrict__ lp_tok,
                                 int* __restrict__ top_id, float* __restrict__ top_lp, VhsLpShared<NT / 64>& sh) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) sh.kmax = 0;
    __syncthreads();
    unsigned km = 0;
    for (int i = tid; i < V; i += NT) km = max(km, vhs_key(row[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) km = max(km, (unsigned)__shfl_xor((int)km, o, 64));
    if (lane == 0) atomicMax(&sh.kmax, km);
    __syncthreads();
    const double M = (double)vhs_unkey(sh.kmax);
    double lse = INFINITY;                  // nothing finite: every log-probability is -inf
    if (M > -INFINITY) {
        double s = 0.0;
        for (int i = tid; i < V; i += NT) s += exp((double)vhs_canon(row[i]) - M);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) sh.part[w] = s;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < NW; ++q) tot += sh.part[q];
        lse = M + log(tot);
    }
    auto lp_of = [&](float v) -> float { return M > -INFINITY ? (float)((double)vhs_canon(v) - lse) : -INFINITY; };
    if (tid == 0 && lp_tok) lp_tok[0] = (tok >= 0 && tok < V) ? lp_of(row[tok]) : -INFINITY;
    if (K <= 0) return;
    unsigned keys[EL > 0 ? EL : 1];          // order keys of this thread's elements (0, below every real key, past V)
    if (EL > 0) {
#pragma unroll
        for (int j = 0; j < EL; ++j) keys[j] = tid + j * NT < V ? vhs_key(row[tid + j * NT]) : 0u;
    }
    unsigned long long prev = ~0ull, mine = 0ull;
    bool rescan = true;
    for (int j = 0; j < K; ++j) {
        if (rescan) {
            mine = 0ull;
            if (EL > 0) {
                // ids ascend with q, so among equal values the first one met is the one to keep: a strict compare of the value keys
                // (and "below the previous winner" among equal values is "a larger id": q * NT > its id - tid, an immediate compare)
                const unsigned ph = (unsigned)(prev >> 32);
                const long long d = (long long)(0xFFFFFFFFu - (unsigned)prev) - tid;
                unsigned mh = 0u;
                int mq = 0;
#pragma unroll
                for (int q = 0; q < EL; ++q) {
                    const unsigned kh = keys[q];
                    if ((kh < ph || (kh == ph && (long long)(q * NT) > d)) && kh > mh) { mh = kh; mq = q; }
                }
                const unsigned ml = 0xFFFFFFFFu - (unsigned)(tid + mq * NT);
                mine = mh ? (((unsigned long long)mh << 32) | ml) : 0ull;
            } else {
                for (int i = tid; i < V; i += NT) {
                    const unsigned long long k = vhs_lp_key(row[i], i);
                    if (k < prev && k > mine) mine = k;
                }
            }
        }
        unsigned long long b = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(b, o, 64); b = t > b ? t : b; }
        __syncthreads();                    // the previous round's sh.top has been read by everyone
        if (lane == 0) sh.top[w] = b;
        __syncthreads();
        b = sh.top[0];
#pragma unroll
        for (int q = 1; q < NW; ++q) b = sh.top[q] > b ? sh.top[q] : b;
        rescan = b != 0ull && mine == b;    // keys are distinct (they carry the id): exactly one owner
        if (tid == 0) {
            if (b == 0ull) { top_id[j] = -1; top_lp[j] = -INFINITY; }
            else { top_id[j] = (int)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFull)); top_lp[j] = lp_of(vhs_unkey((unsigned)(b >> 32))); }
        }
        prev = b;
    }
}
