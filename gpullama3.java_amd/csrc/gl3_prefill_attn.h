// gl3_prefill_attn.h — prefill attention (compiled in gl3_prefill.hip, which keeps the dispatch: pf_attention()).  RoPE + KV write, the per-token
// pair for batches of several sequences, and for ONE sequence's chunk the tiled three-kernel path (scores -> softmax -> weighted V sum) and the
// one-launch kernels (pf_attn_fused_kernel / fused2 / fused3).  Every kernel's LDS size is a constexpr function next to it (*_smem_bytes), and a
// piece that several kernels share is written once:
//   FA_FETCH / FA_PARK      K / V tile staging of the one-launch kernels (global -> named registers -> LDS)
//   FA_SOFTMAX_NUMERATORS / FA_SOFTMAX_DIVIDE       phase 2 of the one-launch kernels
//   SPK_*                   packed-f32 score chains          (pf_scores_pk_kernel, fused2)
//   PK4_PV_TILE             pinned VALU weighted V sum        (pf_pv_ring_kernel, fused2)
//   F3_SCORE_TILE / F3_PV_TILE   MFMA score / weighted-sum chains  (pf_scores_mfma_kernel, pf_pv_mfma_kernel, fused3)
//   Q8_ROUND_PAIR, FA_STORE_ROWS4, g3_scale_operands (gl3_prefill_gemm3.h)     the int8 output epilogues
// They are macros over the calling kernel's own names wherever a function changed the generated code of a kernel.
#pragma once
#include "gl3_prefill_gemm3.h"      // g3_scale_operands: the scale operands of the > 64-token GEMM

typedef float v16f_t __attribute__((ext_vector_type(16)));
typedef float v8f_native __attribute__((ext_vector_type(8)));
typedef float v2f_native __attribute__((ext_vector_type(2)));
typedef float v4f_native_s __attribute__((ext_vector_type(4)));

// LDS any prefill attention kernel may ask for (of the CU's 160 KB): the dispatch conditions and pf_attention_attributes use this one name
constexpr size_t PF_ATTN_LDS_MAX = 150 * 1024;

// ---------------------------------------------------------------------------------------------------
// RoPE on q and k of every token + KV-cache write (batchForwardJavaPrefill :106-121; Qwen3 adds the per-head
// RMSNorm, InferenceCore.java:594-600).  Grid = (n_heads + n_kv_heads, ntok), block = 64.
struct RopeArgs {
    float* QKV; int qkv_stride; float* kcache; float* vcache; const float* cr; const float* ci;
    const float* qnorm; const float* knorm; const float* bq; const float* bk; const float* bv;   // bias: qwen2 (else NULL)
    int n_heads, n_kv_heads, hs, q_dim, kv_dim, arch; float eps;
    const int32_t* seq; const int32_t* pos; size_t seq_stride;   // per-token sequence id / position; floats between sequences' caches
};

__global__ __launch_bounds__(64) void pf_rope_kv_kernel(const RopeArgs a) {
    __shared__ __attribute__((aligned(16))) float v[256];
    const int h = blockIdx.x, b = blockIdx.y, t = threadIdx.x, hs = a.hs;
    const int pos = a.pos[b];
    const size_t soff = (size_t)a.seq[b] * a.seq_stride;
    const bool is_k = h >= a.n_heads;
    const int hk = is_k ? h - a.n_heads : h;
    float* src = a.QKV + (size_t)b * a.qkv_stride + (is_k ? a.q_dim + hk * hs : hk * hs);
    const float* bias = is_k ? a.bk : a.bq;              // qwen2: q / k / v bias before RoPE (InferenceCore.java:456-459)
    for (int i = t; i < hs; i += 64) v[i] = bias ? src[i] + bias[hk * hs + i] : src[i];
    __syncthreads();
    if (a.arch == 1) {
        head_rmsnorm_wave(v, is_k ? a.knorm : a.qnorm, hs, a.eps, t);      // the workgroup is one wavefront
        __syncthreads();
    }
    rope_head(v, hs, a.cr + (size_t)pos * (hs >> 1), a.ci + (size_t)pos * (hs >> 1), a.arch, t, 64);
    __syncthreads();
    if (!is_k) {
        for (int i = t; i < hs; i += 64) src[i] = v[i];
    } else {
        const float* vsrc = a.QKV + (size_t)b * a.qkv_stride + a.q_dim + a.kv_dim + hk * hs;
        for (int i = t; i < hs; i += 64) {
            a.kcache[soff + (size_t)pos * a.kv_dim + hk * hs + i] = v[i];
            a.vcache[soff + (size_t)pos * a.kv_dim + hk * hs + i] = a.bv ? vsrc[i] + a.bv[hk * hs + i] : vsrc[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Batched attention (batchForwardJavaPrefill :123-145: sequential per token, identical arithmetic to decode).
// Scores: grid = (n_tsplit, n_kv_heads, ntok), block = 64 x kvMul; all K rows come from the cache.
struct PfAttnArgs {
    const float* Q; int q_stride;       // roped q rows [ntok][...]
    const float* kcache; const float* vcache;
    float* att;                          // [ntok][n_heads][ctx]
    float* out; int out_stride;          // [ntok][q_dim]
    int n_heads, n_kv_heads, hs, kv_dim, ctx;
    const int32_t* seq; const int32_t* pos; size_t seq_stride;
    float att_mul;                       // 0: score / sqrt(head_size); Granite: score * attentionScale
    int win;                             // pf_attn_softmax_pv_kernel: floats of a softmax row held in LDS (longer rows: windows)
};

__global__ void pf_attn_scores_kernel(const PfAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hs = a.hs, kvmul = a.n_heads / a.n_kv_heads, pitch = hs + 1;
    float* q_s = sm;
    float* kt = q_s + kvmul * hs;
    const int t = threadIdx.x, nthr = blockDim.x;
    const int sp = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int pos = a.pos[b];
    const float* kc = a.kcache + (size_t)a.seq[b] * a.seq_stride;
    const int t0 = sp * ATT_TT;
    if (t0 > pos) return;
    const int t1 = min(pos + 1, t0 + ATT_TT);
    for (int i = t; i < kvmul * hs; i += nthr) q_s[i] = a.Q[(size_t)b * a.q_stride + (kvh * kvmul) * hs + i];
    const int q4 = hs >> 2;
    for (int i = t; i < (t1 - t0) * q4; i += nthr) {
        const int r = i / q4, c = i % q4;
        const float4 v = *reinterpret_cast<const float4*>(kc + (size_t)(t0 + r) * a.kv_dim + kvh * hs + 4 * c);
        float* d = kt + r * pitch + 4 * c;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    const int hq = t >> 6, r = t & 63;
    if (hq < kvmul && t0 + r < t1) {
        const float* q = q_s + hq * hs;
        const float* kk = kt + r * pitch;
        float score = 0.f;
        for (int j = 0; j < hs; ++j) score = score + q[j] * kk[j];
        const float sqrt_hs = (float)sqrt((double)hs);
        a.att[((size_t)b * a.n_heads + kvh * kvmul + hq) * a.ctx + t0 + r] = a.att_mul != 0.f ? score * a.att_mul : score / sqrt_hs;
    }
}

// softmax + weighted V sum: grid = (n_heads * ceil(hs/64), ntok), block = 64.  The row sits in LDS when it fits the window
// (a.win floats); longer rows (contexts beyond ~16 k positions) run in windows: the sequential sum carries its running value
// across them and the numerators are recomputed per window for the weighted V sum (same exp of the same argument -> same bits).
__global__ __launch_bounds__(64) void pf_attn_softmax_pv_kernel(const PfAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float e_s[];
    const int hs = a.hs, kvmul = a.n_heads / a.n_kv_heads;
    const int nj = (hs + 63) / 64;
    const int h = blockIdx.x / nj, j = (blockIdx.x % nj) * 64 + threadIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x, kvh = h / kvmul;
    const int n = a.pos[b] + 1, W = a.win;
    const float* sc = a.att + ((size_t)b * a.n_heads + h) * a.ctx;
    float mx = -INFINITY;
    if (n <= W) { for (int i = lane; i < n; i += 64) { const float s = sc[i]; e_s[i] = s; mx = fmaxf(mx, s); } }
    else { for (int i = lane; i < n; i += 64) mx = fmaxf(mx, sc[i]); }
    mx = wave_max(mx);
    __syncthreads();
    float sum = 0.f;
    if (n <= W) {
        for (int i = lane; i < n; i += 64) e_s[i] = (float)exp((double)(e_s[i] - mx));
        __syncthreads();
        sum = seq_sum_lds<false>(e_s, n);
        __syncthreads();
        for (int i = lane; i < n; i += 64) e_s[i] = e_s[i] / sum;
        __syncthreads();
    } else {
        for (int c0 = 0; c0 < n; c0 += W) {
            const int len = min(W, n - c0);
            __syncthreads();
            for (int i = lane; i < len; i += 64) e_s[i] = (float)exp((double)(sc[c0 + i] - mx));
            __syncthreads();
            sum = seq_sum_lds<false>(e_s, len, sum);
        }
    }
    const float* v = a.vcache + (size_t)a.seq[b] * a.seq_stride + kvh * hs + min(j, hs - 1);
    float acc = 0.f;
    for (int c0 = 0; c0 < n; c0 += W) {                 // one trip unless the row is longer than the window
        const int clen = min(W, n - c0);
        if (n > W) {
            __syncthreads();
            for (int i = lane; i < clen; i += 64) e_s[i] = (float)exp((double)(sc[c0 + i] - mx)) / sum;
            __syncthreads();
        }
        const float* vw = v + (size_t)c0 * a.kv_dim;
        int tt = 0;
        for (; tt + 8 <= clen; tt += 8) {
            float vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) vv[u] = vw[(size_t)(tt + u) * a.kv_dim];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = e_s[tt + u] * vv[u] + acc;
        }
        for (; tt < clen; ++tt) acc = e_s[tt] * vw[(size_t)tt * a.kv_dim] + acc;
    }
    if (j < hs) a.out[(size_t)b * a.out_stride + h * hs + j] = acc;
}

// ---------------------------------------------------------------------------------------------------
// Prefill of ONE sequence (token b sits at position pos0 + b): the K / V tiles are shared by a tile of PA_TB tokens
// instead of being re-read for every token.  Per-element arithmetic and order are those of the per-token kernels above.
//
// Scores: grid = (64-timestep K tiles, n_kv_heads x head groups, token tiles), block = 64 x head slots (min(kvMul, 4): HeadGroup below).  Thread (head hq,
// timestep r) keeps its K row in registers and walks the PA_TB query rows of its head (four chains in flight).
template <int I, int N, int STEP, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + STEP, N, STEP>(f);
    }
}
// maximum over the 64 lanes, uniform result: four DPP steps inside the rows of 16 lanes, then one readlane per row (VALU only; wave_max's
// six ds_bpermute round trips would sit on the score chains' critical path)
#define GL3_DPP_MAX(V_, CTRL_) V_ = fmaxf(V_, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, V_), CTRL_, 0xf, 0xf, false)))
__device__ __forceinline__ float row8_max(float v) {        // every lane: maximum over its aligned group of 8 lanes
    GL3_DPP_MAX(v, 0xB1); GL3_DPP_MAX(v, 0x4E); GL3_DPP_MAX(v, 0x141);      // quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror
    return v;
}
__device__ __forceinline__ float wave_max_uniform(float v) {
    v = row8_max(v); GL3_DPP_MAX(v, 0x140);                                  // row_mirror: the row of 16
    const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float d = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return fmaxf(fmaxf(a, b), fmaxf(c, d));
}
// two score chains advance 16 elements: score = score + q[j] * k[j], j ascending (no FMA)
__device__ __forceinline__ void score_step16(float& s0, float& s1, const v16f_t& qa, const v16f_t& qb, const float4* k) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s0 = s0 + qa[4 * i] * k[i].x;     s1 = s1 + qb[4 * i] * k[i].x;
        s0 = s0 + qa[4 * i + 1] * k[i].y; s1 = s1 + qb[4 * i + 1] * k[i].y;
        s0 = s0 + qa[4 * i + 2] * k[i].z; s1 = s1 + qb[4 * i + 2] * k[i].z;
        s0 = s0 + qa[4 * i + 3] * k[i].w; s1 = s1 + qb[4 * i + 3] * k[i].w;
    }
}
constexpr int PA_TB = 16;
// The token tile of a workgroup of the long-context kernels (scores / weighted V sum over score rows in HBM).  One sequence (TAB = false): tile
// `tile` of TB rows of the chunk, (pos0, ntok) from the arguments.  Run-table form (TAB = true, the deep rows of a mixed step of
// gl3_forward_batch): `tile` picks a record {first row, rows <= 16, sequence, position of the first row} of the step's deep table
// (gl3_batch_plan.h: batch_plan_split); the caches move to the record's sequence and pos0 becomes position - row, so that everything behind
// this prologue — "row b of the step sits at position pos0 + b", the clamps, the per-tile maxima, the e / sum staging — is the one-sequence
// code unchanged, with ATT / TMX / SUMS indexed by step row.  `tile` is a blockIdx component: the record arrives by a scalar load and the
// four values are wavefront-uniform (SGPRs), as in fa_tile of the one-launch kernels.
struct LcTile { int b0, nb, pos0; size_t cache_off; };           // cache_off: floats from the caches' base to the tile's sequence
template <bool TAB, int TB>
__device__ __forceinline__ LcTile lc_tile(int tile, int pos0, int ntok, const int4* __restrict__ tab, size_t seq_stride) {
    LcTile r;
    if constexpr (TAB) {
        const int4 rec = tab[tile];
        r.b0 = __builtin_amdgcn_readfirstlane(rec.x); r.nb = __builtin_amdgcn_readfirstlane(rec.y);
        r.cache_off = (size_t)__builtin_amdgcn_readfirstlane(rec.z) * seq_stride;
        r.pos0 = __builtin_amdgcn_readfirstlane(rec.w) - r.b0;
    } else {
        r.b0 = tile * TB; r.nb = min(TB, ntok - r.b0); r.pos0 = pos0; r.cache_off = 0;
    }
    return r;
}
// The head group of a workgroup of the tiled kernels.  A kv head's kvMul query heads are served `slots` = min(kvMul, 4) consecutive heads at a time:
// NG = ceil(kvMul / slots) groups, the last of which holds 1 .. slots real heads (kvMul <= 4: one group, every slot real).  Head slot hq of
// group g is the head h0 + hq; a surplus slot of a ragged last group points at the group's last real head (head_of: never a head of another
// kv head), computes what that head's slot computes, reaches every barrier and stores nothing (real).  The group index is a grid component
// beside the token tile of fa_tile / lc_tile — blockIdx.y of the one-launch kernels, folded into the kv-head component (kvh * NG + g) of the
// long-context kernels, whose three grid components are taken — so it is wavefront-uniform and everything here stays in SGPRs.
struct HeadGroup {
    int kvh, h0, nh;                                             // kv head, first head of the group, real heads in it
    __device__ __forceinline__ int head_of(int hq) const { return h0 + min(hq, nh - 1); }
    __device__ __forceinline__ bool real(int hq) const { return hq < nh; }
};
__device__ __forceinline__ HeadGroup head_group(int kvh, int g, int kvmul, int slots) {
    HeadGroup r; r.kvh = kvh; r.h0 = kvh * kvmul + slots * g; r.nh = min(slots, kvmul - slots * g);
    return r;
}
__device__ __forceinline__ HeadGroup lc_head_group(int kg, int kvmul, int slots) {      // kg = kvh * NG + g
    const int ng = (kvmul + slots - 1) / slots, kvh = __builtin_amdgcn_readfirstlane(kg / ng);
    return head_group(kvh, kg - kvh * ng, kvmul, slots);
}
template <int HS, bool TAB = false>
__global__ __launch_bounds__(256) void pf_scores_tiled_kernel(const float* __restrict__ Q, int q_stride, const float* __restrict__ kc,
                                                              float* __restrict__ att, int n_heads, int kvmul, int kv_dim, int ctx,
                                                              int pos0, int ntok, float att_mul, float* __restrict__ tmx, int tmx_tiles,
                                                              const int4* __restrict__ tab = nullptr, size_t seq_stride = 0) {
    extern __shared__ __attribute__((aligned(16))) float kt[];       // [64][PITCH]
    constexpr int PITCH = HS + 4, H4 = HS / 4;
    const int t = threadIdx.x, nthr = blockDim.x;
    const LcTile lt = lc_tile<TAB, PA_TB>(blockIdx.z, pos0, ntok, tab, seq_stride);
    const HeadGroup hg = lc_head_group(blockIdx.y, kvmul, nthr >> 6);      // one wavefront per head slot
    const int t0 = blockIdx.x * 64, kvh = hg.kvh, b0 = lt.b0, nb = lt.nb;
    pos0 = lt.pos0; kc += lt.cache_off;               // of the tile's sequence from here on
    const int tmax = pos0 + b0 + nb - 1;              // last timestep any token of this tile attends to
    if (tmax < t0) return;
    const int t1 = min(tmax + 1, t0 + 64);
    for (int i = t; i < (t1 - t0) * H4; i += nthr) {
        const int r = i / H4, c = i % H4;
        *reinterpret_cast<float4*>(kt + r * PITCH + 4 * c) =
            *reinterpret_cast<const float4*>(kc + (size_t)(t0 + r) * kv_dim + kvh * HS + 4 * c);
    }
    __syncthreads();
    const int hq = __builtin_amdgcn_readfirstlane(t >> 6), r = t & 63;
    float4 kr[H4];
#pragma unroll
    for (int c = 0; c < H4; ++c) kr[c] = *reinterpret_cast<const float4*>(kt + min(r, t1 - t0 - 1) * PITCH + 4 * c);
    const float sqrt_hs = (float)sqrt((double)HS);
    const int head = hg.head_of(hq);
    const bool hreal = hg.real(hq);
    for (int tb = 0; tb < nb; tb += 2) {
        // the two query rows are wavefront-uniform: scalar loads (8 floats per row per step, double-buffered), SGPR
        // operands in the multiplies.  Explicit s_load: the compiler would hoist every load and spill SGPRs.
        const float* q0 = Q + (size_t)(b0 + tb) * q_stride + (size_t)head * HS;
        const float* q1 = Q + (size_t)(b0 + min(tb + 1, nb - 1)) * q_stride + (size_t)head * HS;
        float s0 = 0.f, s1 = 0.f;
        if constexpr (HS >= 64) {
            v16f_t a0, a1, c0, c1;                    // 16 q values per row per step (64 SGPRs for the double buffer)
            asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %3, 0x0" : "=&s"(a0), "=&s"(a1) : "s"(q0), "s"(q1));
            static_for<0, H4 / 4, 2>([&](auto ic) {
                constexpr int c4 = decltype(ic)::value;
                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+v"(s0), "+v"(s1));   // s0/s1 pin the VALU chain between the asm statements
                asm volatile("s_load_dwordx16 %0, %2, %4\n\ts_load_dwordx16 %1, %3, %4" : "=&s"(c0), "=&s"(c1) : "s"(q0), "s"(q1), "n"((c4 + 1) * 64));
                score_step16(s0, s1, a0, a1, &kr[4 * c4]);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(c0), "+s"(c1), "+v"(s0), "+v"(s1));
                if constexpr (c4 + 2 < H4 / 4)
                    asm volatile("s_load_dwordx16 %0, %2, %4\n\ts_load_dwordx16 %1, %3, %4" : "=&s"(a0), "=&s"(a1) : "s"(q0), "s"(q1), "n"((c4 + 2) * 64));
                score_step16(s0, s1, c0, c1, &kr[4 * c4 + 4]);
            });
        } else {
            v16f_t a0, a1, c0, c1;
            asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %3, 0x0" : "=&s"(a0), "=&s"(a1) : "s"(q0), "s"(q1));
            asm volatile("s_load_dwordx16 %0, %2, 64\n\ts_load_dwordx16 %1, %3, 64" : "=&s"(c0), "=&s"(c1) : "s"(q0), "s"(q1));
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+s"(c0), "+s"(c1), "+v"(s0), "+v"(s1));
            score_step16(s0, s1, a0, a1, &kr[0]);
            score_step16(s0, s1, c0, c1, &kr[4]);
        }
        const int b = b0 + tb;
        const float v0 = att_mul != 0.f ? s0 * att_mul : s0 / sqrt_hs, v1 = att_mul != 0.f ? s1 * att_mul : s1 / sqrt_hs;
        const bool ok0 = hreal && t0 + r <= pos0 + b, ok1 = hreal && tb + 1 < nb && t0 + r <= pos0 + b + 1;       // (tmax >= pos0 + b: both imply t0 + r < t1)
        if (ok0) att[((size_t)b * n_heads + head) * ctx + t0 + r] = v0;
        if (ok1) att[((size_t)(b + 1) * n_heads + head) * ctx + t0 + r] = v1;
        if (tmx) {      // r6: the tile's maximum per (token, head) row for pf_softmax_rows_kernel (max is order-independent)
            const float m0 = wave_max_uniform(ok0 ? v0 : -INFINITY), m1 = wave_max_uniform(ok1 ? v1 : -INFINITY);
            if (r == 0 && hreal) {
                if (t0 <= pos0 + b) tmx[((size_t)b * n_heads + head) * tmx_tiles + blockIdx.x] = m0;
                if (tb + 1 < nb && t0 <= pos0 + b + 1) tmx[((size_t)(b + 1) * n_heads + head) * tmx_tiles + blockIdx.x] = m1;
            }
        }
    }
}

// r6 — pf_scores_tiled_kernel on packed f32: two tokens' chains advance in ONE register pair, {s_a, s_b} = {s_a, s_b} + {q_a[j], q_b[j]} * k[j]
// (v_pk_mul_f32 + v_pk_add_f32: every product and every sum rounded as before, j ascending), two pairs side by side per wavefront.  The query
// rows of the tile's 16 tokens reach LDS once per workgroup, interleaved by token pairs ([head][pair][j][2]), so a 16-byte broadcast read is
// two steps of a pair; the reads of the next group of 8 steps are pinned under the current group's 32 packed instructions.  (The scalar-load
// form feeds q through SGPRs: its lead is bounded by the SGPR file — one group of 16 steps — and the scalar cache misses to L2 at 32 KB of
// query rows per workgroup.)  K rows in registers as before, lane = timestep.  Two wavefronts per SIMD (~210 VGPRs, 65 KB of LDS).
__host__ __device__ constexpr size_t scores_tiled_smem_bytes(int hs) { return (size_t)64 * (hs + 4) * 4; }                     // pf_scores_tiled_kernel: the K tile
__host__ __device__ constexpr size_t scores_pk_smem_bytes(int hs, int kvmul) { return scores_tiled_smem_bytes(hs) + (size_t)kvmul * PA_TB * hs * 4; }
template <int HS, int KVM, bool TAB = false>
__global__ __launch_bounds__(64 * KVM) __attribute__((amdgpu_waves_per_eu(2, 2))) void pf_scores_pk_kernel(const float* __restrict__ Q, int q_stride, const float* __restrict__ kc,
        float* __restrict__ att, int n_heads, int kvmul, int kv_dim, int ctx, int pos0, int ntok, float att_mul, float* __restrict__ tmx, int tmx_tiles,
        const int4* __restrict__ tab = nullptr, size_t seq_stride = 0) {
    extern __shared__ __attribute__((aligned(16))) float kt[];       // [64][PITCH] K rows, then [KVM][8 pairs][HS][2] query rows
    constexpr int PITCH = HS + 4, H4 = HS / 4, NGR = HS / 8, NT = 64 * KVM, KPT = 64 * H4 / NT, QPT = H4 / 8;
    static_assert(KPT * NT == 64 * H4 && QPT * 8 == H4, "staging slots per thread");
    float* qs = kt + 64 * PITCH;
    const int t = threadIdx.x;
    const LcTile lt = lc_tile<TAB, PA_TB>(blockIdx.z, pos0, ntok, tab, seq_stride);
    const HeadGroup hg = lc_head_group(blockIdx.y, kvmul, KVM);      // KVM head slots of the kv head's kvmul query heads
    const int t0 = blockIdx.x * 64, kvh = hg.kvh, b0 = lt.b0, nb = lt.nb;
    pos0 = lt.pos0; kc += lt.cache_off;               // of the tile's sequence from here on
    const int tmax = pos0 + b0 + nb - 1;
    if (tmax < t0) return;
    const int t1 = min(tmax + 1, t0 + 64);
    {   // staging: EVERY global load of the workgroup's K tile and query rows is in flight before the first LDS write (a loop with a run-time
        // trip count keeps one load per thread in flight: 8 + 8 L2 round trips per workgroup against ~8 us of arithmetic)
        v4f_native_s kreg[KPT], qra[QPT], qrb[QPT];
#pragma unroll
        for (int j = 0; j < KPT; ++j) {                               // rows past the tile's last timestep repeat it (their scores are never stored)
            const int i = t + NT * j, r = i / H4, c = i % H4;
            kreg[j] = *reinterpret_cast<const v4f_native_s*>(kc + (size_t)(t0 + min(r, t1 - t0 - 1)) * kv_dim + kvh * HS + 4 * c);
        }
#pragma unroll
        for (int j = 0; j < QPT; ++j) {                               // slot = (head, token pair, 4 columns): both tokens' float4
            const int i = t + NT * j, c = i % H4, pair = (i / H4) % (PA_TB / 2), hq = i / (H4 * (PA_TB / 2));
            const float* qp = Q + (size_t)hg.head_of(hq) * HS + 4 * c;
            qra[j] = *reinterpret_cast<const v4f_native_s*>(qp + (size_t)(b0 + min(2 * pair, nb - 1)) * q_stride);
            qrb[j] = *reinterpret_cast<const v4f_native_s*>(qp + (size_t)(b0 + min(2 * pair + 1, nb - 1)) * q_stride);
        }
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const int i = t + NT * j, r = i / H4, c = i % H4;
            *reinterpret_cast<v4f_native_s*>(kt + r * PITCH + 4 * c) = kreg[j];
        }
#pragma unroll
        for (int j = 0; j < QPT; ++j) {
            const int i = t + NT * j, c = i % H4, pair = (i / H4) % (PA_TB / 2), hq = i / (H4 * (PA_TB / 2));
            float* d = qs + ((size_t)(hq * (PA_TB / 2) + pair) * HS + 4 * c) * 2;
            *reinterpret_cast<v4f_native_s*>(d) = (v4f_native_s){qra[j].x, qrb[j].x, qra[j].y, qrb[j].y};
            *reinterpret_cast<v4f_native_s*>(d + 4) = (v4f_native_s){qra[j].z, qrb[j].z, qra[j].w, qrb[j].w};
        }
    }
    __syncthreads();
    const int hq = __builtin_amdgcn_readfirstlane(t >> 6), r = t & 63;
    v2f_native kr[HS / 2];                                             // this lane's K row as 64-bit operands {k[2 i], k[2 i + 1]}
#pragma unroll
    for (int c = 0; c < H4; ++c) {
        const v4f_native_s x = *reinterpret_cast<const v4f_native_s*>(kt + r * PITCH + 4 * c);
        kr[2 * c] = x.xy; kr[2 * c + 1] = x.zw;
    }
    const float sqrt_hs = (float)sqrt((double)HS);
    const int head = hg.head_of(hq);
    const bool hreal = hg.real(hq);
    for (int pp = 0; 4 * pp < nb; ++pp) {
        const float* q01 = qs + (size_t)(hq * (PA_TB / 2) + 2 * pp) * HS * 2;      // pairs (4 pp, 4 pp + 1) and (4 pp + 2, 4 pp + 3)
        const float* q23 = q01 + HS * 2;
        v2f_native c0 = {0.f, 0.f}, c1 = {0.f, 0.f};
        v4f_native_s qa[8], qb[8];                                     // two groups of 8 steps: [0..3] pair 0, [4..7] pair 1
#define SPK_LD(G_, R_) do { _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) { \
            R_[i_] = *reinterpret_cast<const v4f_native_s*>(q01 + 16 * (G_) + 4 * i_); R_[4 + i_] = *reinterpret_cast<const v4f_native_s*>(q23 + 16 * (G_) + 4 * i_); } } while (0)
        // two steps of both pairs in one block: the K value is broadcast out of its register pair by op_sel (the compiler materialises {k, k}
        // pairs instead: twice the K registers), and every dependent instruction has an independent one in front of it (packed f32 needs a wait
        // state between a result and its use)
#define SPK_STEP2(QA_, QB_, K_) do { v2f_native p0_, p1_; \
            asm("v_pk_mul_f32 %[p0], %[qa0], %[k] op_sel_hi:[1,0]\n\tv_pk_mul_f32 %[p1], %[qb0], %[k] op_sel_hi:[1,0]\n\t" \
                "v_pk_add_f32 %[c0], %[c0], %[p0]\n\tv_pk_add_f32 %[c1], %[c1], %[p1]\n\t" \
                "v_pk_mul_f32 %[p0], %[qa1], %[k] op_sel:[0,1]\n\tv_pk_mul_f32 %[p1], %[qb1], %[k] op_sel:[0,1]\n\t" \
                "v_pk_add_f32 %[c0], %[c0], %[p0]\n\tv_pk_add_f32 %[c1], %[c1], %[p1]" \
                : [c0] "+v"(c0), [c1] "+v"(c1), [p0] "=&v"(p0_), [p1] "=&v"(p1_) \
                : [qa0] "v"(QA_.xy), [qa1] "v"(QA_.zw), [qb0] "v"(QB_.xy), [qb1] "v"(QB_.zw), [k] "v"(K_)); } while (0)
#define SPK_ACC(G_, R_) do { SPK_STEP2(R_[0], R_[4], kr[4 * (G_)]); SPK_STEP2(R_[1], R_[5], kr[4 * (G_) + 1]); \
            SPK_STEP2(R_[2], R_[6], kr[4 * (G_) + 2]); SPK_STEP2(R_[3], R_[7], kr[4 * (G_) + 3]); } while (0)
        SPK_LD(0, qa); SPK_LD(1, qb); __builtin_amdgcn_sched_barrier(0);
        static_for<0, NGR, 2>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            SPK_ACC(g, qa);
            SPK_LD((g + 2 < NGR ? g + 2 : NGR - 1), qa); __builtin_amdgcn_sched_barrier(0);
            SPK_ACC(g + 1, qb);
            SPK_LD((g + 3 < NGR ? g + 3 : NGR - 1), qb); __builtin_amdgcn_sched_barrier(0);
        });
        const float sv[4] = {c0.x, c0.y, c1.x, c1.y};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int tb = 4 * pp + u, b = b0 + tb;
            const float v = att_mul != 0.f ? sv[u] * att_mul : sv[u] / sqrt_hs;
            const bool ok = hreal && tb < nb && t0 + r <= pos0 + b;
            if (ok) att[((size_t)b * n_heads + head) * ctx + t0 + r] = v;
            if (tmx) {
                const float m = wave_max_uniform(ok ? v : -INFINITY);
                if (r == 0 && hreal && tb < nb && t0 <= pos0 + b) tmx[((size_t)b * n_heads + head) * tmx_tiles + blockIdx.x] = m;
            }
        }
    }
}

// r6 — softmax of the score rows at depth, R rows per workgroup: 8 worker wavefronts stream the rows' 64-timestep tiles (loads a tile ahead,
// e_t = (float) exp((double) (s_t - max)) written back in place and into a double-buffered LDS tile), a ninth wavefront runs the strictly
// sequential sums with lane = row — R chains side by side, LDS reads pinned ahead of the adds (seq_sum_lds_ring).  The row maxima come from
// the per-tile maxima pf_scores_tiled_kernel leaves in tmx (max is order-independent); the denominators go to `sums` and the division
// e_t / sum happens where the weights are staged (pf_pv_mfma_kernel / pf_pv_ring_kernel) — same operands, same rounding as
// FloatTensor.softmaxInPlace (J/tensor/standard/FloatTensor.java:196-219: max, exp, sum, divide).  Needs ctx % 4 == 0 (16-byte row starts).
// `rows` (null: every row of the step, row i = (token i / n_heads, head i % n_heads)): the deep step rows of a mixed step, ascending — the launch
// covers rows x n_heads score rows and touches ATT / TMX / SUMS of those step rows only (a shallow row's were not written in this step).
constexpr int SR_PITCH = 68;
template <int R>
__global__ __launch_bounds__(576) void pf_softmax_rows_kernel(const PfAttnArgs a, int nrows_total, const float* __restrict__ tmx, int tmx_tiles, float* __restrict__ sums,
                                                              const int32_t* __restrict__ rows = nullptr) {
    __shared__ __attribute__((aligned(16))) float E[2][R * SR_PITCH];
    __shared__ float mx_s[R];
    __shared__ int n_s[R];
    __shared__ int row_s[R];                          // the (step row, head) score row of the workgroup's row r
    __shared__ int nmax_s;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int row0 = blockIdx.x * R;
    if (t == 0) nmax_s = 0;
    if (t < R * 8) {                                  // 8 lanes fold a row's tile maxima
        const int r = t >> 3, sub = t & 7, lrow = min(row0 + r, nrows_total - 1);
        const int row = rows ? rows[lrow / a.n_heads] * a.n_heads + lrow % a.n_heads : lrow;
        const int n = row0 + r < nrows_total ? a.pos[row / a.n_heads] + 1 : 0;
        const int nt = (n + 63) >> 6;
        float m = -INFINITY;
        for (int i = sub; i < nt; i += 8) m = fmaxf(m, tmx[(size_t)row * tmx_tiles + i]);
        m = row8_max(m);
        if (sub == 0) { mx_s[r] = m; n_s[r] = n; row_s[r] = row; }
    }
    __syncthreads();
    if (t < R) atomicMax(&nmax_s, n_s[t]);
    __syncthreads();
    const int ntile = (nmax_s + 63) >> 6;
    if (wave == 8) {                                  // the chains: lane = row
        const int r = min(lane, R - 1);
        float s = 0.f;
        for (int k = 0; k < ntile; ++k) {
            __syncthreads();                          // tile k has landed in E[k & 1]; the workers refill it behind the NEXT barrier
            s = seq_sum_lds_ring(&E[k & 1][r * SR_PITCH], 64, s);
        }
        if (lane < R && row0 + lane < nrows_total) sums[row_s[lane]] = s;
        return;
    }
    constexpr int NS = (R * 16 + 511) / 512;          // 16-byte slots per worker thread and tile
    float* rowp[NS]; float mrow[NS]; int nrow[NS], ldsoff[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const int q = min(t + 512 * u, R * 16 - 1), r = q >> 4, c4 = q & 15;
        rowp[u] = a.att + (size_t)row_s[r] * a.ctx + 4 * c4;
        mrow[u] = mx_s[r];
        nrow[u] = (t + 512 * u < R * 16) ? n_s[r] - 4 * c4 : 0;       // elements of the row at and behind this slot's first column of tile 0
        ldsoff[u] = r * SR_PITCH + 4 * c4;
    }
    float4 cur[NS], nxt[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) cur[u] = *reinterpret_cast<const float4*>(rowp[u]);               // tile 0 (column 4 c4 < 64 <= ctx)
    for (int k = 0; k < ntile; ++k) {
        const int kn = min(k + 1, ntile - 1);
#pragma unroll
        for (int u = 0; u < NS; ++u) {                // unconditional loads: slots past the row's end re-read tile 0 (masked below)
            const float* src = 64 * kn < nrow[u] ? rowp[u] + 64 * kn : rowp[u];
            nxt[u] = *reinterpret_cast<const float4*>(src);
        }
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const int left = nrow[u] - 64 * k;        // valid elements of this slot: min(left, 4)
            float4 e;
            e.x = left > 0 ? (float)exp((double)(cur[u].x - mrow[u])) : 0.f;
            e.y = left > 1 ? (float)exp((double)(cur[u].y - mrow[u])) : 0.f;
            e.z = left > 2 ? (float)exp((double)(cur[u].z - mrow[u])) : 0.f;
            e.w = left > 3 ? (float)exp((double)(cur[u].w - mrow[u])) : 0.f;
            if (t + 512 * u < R * 16) *reinterpret_cast<float4*>(&E[k & 1][ldsoff[u]]) = e;
            if (left > 0) *reinterpret_cast<float4*>(rowp[u] + 64 * k) = e;      // in place (columns past the row's end stay inside the row: ctx % 4 == 0)
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NS; ++u) cur[u] = nxt[u];
    }
}

// r6 — the weighted V sum on the VALU: grid = (n_heads, token tiles of 32), V tiles of 64 timesteps through LDS, wavefront = 4 tokens, lane = the
// output column(s): acc = a_t * v + acc, t ascending.  Two latencies are off the critical path:
//   * the NEXT tile's V rows and softmax numerators are requested into registers before the current tile is consumed and reach LDS behind it;
//   * inside a tile the LDS reads of timestep group g + 1 (four weights per token, four V rows) are in flight under the 64 multiply-add pairs
//     of group g, pinned there with sched_barrier (left alone the scheduler sinks every read next to its use).
// Masking is by weight: timesteps behind a token's position get the weight 0 (0 * v + acc = acc exactly: acc is never -0 and every staged
// V row is a written row <= the tile's last position), so the inner loop has no per-token conditions.  The division e_t / sum happens
// where the weights are staged (sums from pf_softmax_rows_kernel).
constexpr int PVR_NW = 8, PVR_TB = 4 * PVR_NW;     // 8 wavefronts of 4 tokens: a V tile serves 32 tokens, 512 workgroups for 512 tokens x 32 heads (two per CU)
// The weighted V sum of one 64-timestep tile on the VALU (pf_pv_ring_kernel and phase 3 of pf_attn_fused2_kernel): groups of four timesteps, the
// next group's weights and V rows are read from LDS under the current group's 64 multiply-add pairs (pinned with sched_barrier: left alone the
// scheduler sinks every read next to its use).  Timesteps behind a token's position carry the weight 0, so there are no per-token conditions.
// In scope: acc[4][NCOL]; ap = the weights of the wavefront's first token at the tile's first timestep, the four tokens' rows WP_ floats apart;
// vp = the lane's column(s) of the tile's first V row, rows VP_ floats apart.  NG_ = groups of four timesteps the wavefront's tokens reach.
#define PVR_LD(G_, WP_, VP_, W0_, W1_, W2_, W3_, V_) do { const int r_ = 4 * min((G_), 15); \
            W0_ = *reinterpret_cast<const float4*>(ap + r_); W1_ = *reinterpret_cast<const float4*>(ap + (size_t)(WP_) + r_); \
            W2_ = *reinterpret_cast<const float4*>(ap + 2 * (size_t)(WP_) + r_); W3_ = *reinterpret_cast<const float4*>(ap + 3 * (size_t)(WP_) + r_); \
            _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) { \
                if (NCOL == 2) { const float2 x_ = *reinterpret_cast<const float2*>(vp + (r_ + i_) * (VP_)); V_[i_][0] = x_.x; V_[i_][NCOL - 1] = x_.y; } \
                else V_[i_][0] = vp[(r_ + i_) * (VP_)]; } } while (0)
#define PVR_STEP(I_, WX_, V_, W0_, W1_, W2_, W3_) do { const float w_[4] = {W0_.WX_, W1_.WX_, W2_.WX_, W3_.WX_}; \
            _Pragma("unroll") for (int u_ = 0; u_ < 4; ++u_) _Pragma("unroll") for (int c_ = 0; c_ < NCOL; ++c_) acc[u_][c_] = w_[u_] * V_[I_][c_] + acc[u_][c_]; } while (0)
#define PVR_ACC(V_, W0_, W1_, W2_, W3_) do { PVR_STEP(0, x, V_, W0_, W1_, W2_, W3_); PVR_STEP(1, y, V_, W0_, W1_, W2_, W3_); \
            PVR_STEP(2, z, V_, W0_, W1_, W2_, W3_); PVR_STEP(3, w, V_, W0_, W1_, W2_, W3_); } while (0)
#define PVR_TILE(NG_, WP_, VP_) do { const int ng_ = (NG_); \
        float4 wa0, wa1, wa2, wa3, wb0, wb1, wb2, wb3; \
        float va[4][NCOL], vb4[4][NCOL]; \
        PVR_LD(0, WP_, VP_, wa0, wa1, wa2, wa3, va); PVR_LD(1, WP_, VP_, wb0, wb1, wb2, wb3, vb4); __builtin_amdgcn_sched_barrier(0); \
        int g = 0; \
        for (; g + 2 <= ng_; g += 2) { \
            PVR_ACC(va, wa0, wa1, wa2, wa3); \
            PVR_LD(g + 2, WP_, VP_, wa0, wa1, wa2, wa3, va); __builtin_amdgcn_sched_barrier(0); \
            PVR_ACC(vb4, wb0, wb1, wb2, wb3); \
            PVR_LD(g + 3, WP_, VP_, wb0, wb1, wb2, wb3, vb4); __builtin_amdgcn_sched_barrier(0); \
        } \
        if (g < ng_) PVR_ACC(va, wa0, wa1, wa2, wa3); } while (0)
__host__ __device__ constexpr size_t pv_ring_smem_bytes(int hs) { return (size_t)64 * (hs + PVR_TB) * 4; }
template <int HS, bool TAB = false>
__global__ __launch_bounds__(64 * PVR_NW) void pf_pv_ring_kernel(const PfAttnArgs a, int seq, int pos0, int ntok, const float* __restrict__ sums,
                                                                const int4* __restrict__ tab = nullptr) {
    constexpr int NCOL = HS > 64 ? 2 : 1, H4 = HS / 4, NT = 64 * PVR_NW, VPT = 64 * H4 / NT;
    static_assert(VPT * NT == 64 * H4, "a V tile is a whole number of 16-byte slots per thread");
    extern __shared__ __attribute__((aligned(16))) float vt[];        // [64][HS] V rows, then [PVR_TB][64] weights
    float* as = vt + 64 * HS;
    const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    // table form: one deep record (<= 16 rows) per workgroup; wavefronts 4 - 7 see 4 w >= nb and idle through wmax = -1
    const LcTile lt = lc_tile<TAB, PVR_TB>(blockIdx.y, pos0, ntok, tab, a.seq_stride);
    const int kvmul = a.n_heads / a.n_kv_heads, h = blockIdx.x, kvh = h / kvmul, b0 = lt.b0, nb = lt.nb;
    pos0 = lt.pos0;
    const int tmax = pos0 + b0 + nb - 1, ntile = tmax / 64 + 1;
    const int wmax = 4 * w < nb ? pos0 + b0 + min(4 * w + 3, nb - 1) : -1;     // last position any of this wavefront's four tokens attends to
    const float* vc = a.vcache + (TAB ? lt.cache_off : (size_t)seq * a.seq_stride) + kvh * HS;
    // staging roles: thread = (token w + PVR_NW j, timestep lane) of the weights; 16-byte slots t + NT j of the V tile
    const float* arow[4]; float rsum[4]; int apos[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tb = w + PVR_NW * j;
        apos[j] = tb < nb ? pos0 + b0 + tb : -1;
        arow[j] = a.att + ((size_t)(b0 + min(tb, nb - 1)) * a.n_heads + h) * a.ctx;
        rsum[j] = sums[(size_t)(b0 + min(tb, nb - 1)) * a.n_heads + h];
    }
    typedef float v4f_native __attribute__((ext_vector_type(4)));     // typed loads / stores (a float4 array that is only copied in and out stays a stack object)
    v4f_native vreg[VPT]; float areg[4];
#define PVR_GLOAD(K_) do { const int t0_ = 64 * (K_); \
        static_for<0, VPT, 1>([&](auto jc) { constexpr int j = decltype(jc)::value; const int i = t + NT * j, r = i / H4, c = i % H4; \
            vreg[j] = *reinterpret_cast<const v4f_native*>(vc + (size_t)min(t0_ + r, tmax) * a.kv_dim + 4 * c); }); \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) areg[j] = arow[j][max(min(t0_ + lane, apos[j]), 0)]; } while (0)
#define PVR_LSTORE(K_) do { const int t0_ = 64 * (K_); \
        static_for<0, VPT, 1>([&](auto jc) { constexpr int j = decltype(jc)::value; const int i = t + NT * j, r = i / H4, c = i % H4; \
            *reinterpret_cast<v4f_native*>(vt + r * HS + 4 * c) = vreg[j]; }); \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) as[(w + PVR_NW * j) * 64 + lane] = t0_ + lane <= apos[j] ? areg[j] / rsum[j] : 0.f; } while (0)
    float acc[4][NCOL];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < NCOL; ++c) acc[u][c] = 0.f;
    const float* vp = vt + (NCOL == 2 ? 2 * min(lane, HS / 2 - 1) : min(lane, HS - 1));      // lanes past the last column (head size 96, 32) repeat it and store nothing
    const float* ap = as + 4 * w * 64;
    PVR_GLOAD(0);
    PVR_LSTORE(0);
    __syncthreads();
    for (int k = 0; k < ntile; ++k) {
        PVR_GLOAD(min(k + 1, ntile - 1));                            // unconditional (a condition around the loads makes the compiler drain them)
        const int ng = max(0, min(64, wmax + 1 - 64 * k) + 3) >> 2;   // groups of four timesteps this wavefront's tokens reach in the tile
        PVR_TILE(ng, 64, HS);
        __syncthreads();
        PVR_LSTORE(min(k + 1, ntile - 1));
        __syncthreads();
    }
#undef PVR_GLOAD
#undef PVR_LSTORE
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int tb = 4 * w + u;
        if (tb >= nb) continue;
#pragma unroll
        for (int c = 0; c < NCOL; ++c) {
            const int j = NCOL == 2 ? 2 * lane + c : lane;
            if (j < HS) a.out[(size_t)(b0 + tb) * a.out_stride + h * HS + j] = acc[u][c];
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Round 4: scores + softmax + weighted V sum of ONE sequence's prefill chunk in one launch (the three kernels above stay for long
// contexts and odd shapes).  Workgroup = (kv head, tile of FA_TB = 8 tokens), 2 * kvMul wavefronts; the score rows of the tile's
// kvMul x 8 (query head, token) pairs live in LDS from the first q.k to the last a.v — no [token][head][ctx] round trip through
// HBM / L2 (33 MB written, read, rewritten and read again per 8B layer at 512 tokens) and one launch instead of three.
//   phase 1  scores: the K tiles of 64 timesteps alternate between the two wavefront groups; thread = (query head, timestep), K row
//            in registers, the query rows as SGPR operands (pf_scores_tiled_kernel's inner loop: j ascending, product rounded, no FMA)
//   phase 2  softmax rows (FloatTensor.softmaxInPlace): max, exp in double, the strictly sequential sum of ALL rows at once
//            (lane = row: 32 chains side by side instead of one row per wavefront), divide
//   phase 3  weighted V sum: V tiles of 64 timesteps through LDS, wavefront = (query head, 4 tokens), lane = 2 columns,
//            acc = a_t * v + acc with t ascending
// Tiles are dealt heaviest (latest positions) first, so the triangular work profile does not leave a tail.
constexpr int FA_TB = 8;
// (kvmul of the *_smem_bytes functions: the head slots of a workgroup — the head group's size min(kvMul, 4), HeadGroup above)
__host__ __device__ constexpr size_t fa_smem_bytes(int hs, int kvmul, int sstride) {
    return ((size_t)kvmul * FA_TB * sstride + 2 * 64 * (hs + 4) + 64) * 4;
}
// The (kv head, token tile) of a workgroup of the one-launch kernels.  One sequence (TAB = false): tiles of FA_TB rows of the chunk, dealt
// heaviest first from blockIdx and (pos0, ntok).  Run-table form (TAB = true, a mixed step of gl3_forward_batch): blockIdx / n_kv_heads picks a
// record {first row, rows, sequence, position of the first row} of the step's tile table (gl3_batch_plan.h, already ordered deepest first);
// the caches move to the record's sequence and pos0 becomes position - row, so that everything behind this prologue — "row b of the step sits
// at position pos0 + b" — is the one-sequence code unchanged.  The record's address depends on blockIdx alone: it arrives by a scalar load
// and the four values are wavefront-uniform (SGPRs), like the arithmetic on blockIdx they replace.
struct FaTile { int kvh, g, b0, nb, pos0; size_t cache_off; };   // g: head group (blockIdx.y); cache_off: floats from the caches' base to the tile's sequence
template <bool TAB>
__device__ __forceinline__ FaTile fa_tile(int n_kv_heads, int pos0, int ntok, const int4* __restrict__ tab, size_t seq_stride) {
    FaTile r;
    r.kvh = blockIdx.x % n_kv_heads; r.g = blockIdx.y;
    if constexpr (TAB) {
        const int4 rec = tab[blockIdx.x / n_kv_heads];
        r.b0 = __builtin_amdgcn_readfirstlane(rec.x); r.nb = __builtin_amdgcn_readfirstlane(rec.y);
        r.cache_off = (size_t)__builtin_amdgcn_readfirstlane(rec.z) * seq_stride;
        r.pos0 = __builtin_amdgcn_readfirstlane(rec.w) - r.b0;
    } else {
        const int ntile = (ntok + FA_TB - 1) / FA_TB, tile = ntile - 1 - blockIdx.x / n_kv_heads;
        r.b0 = tile * FA_TB; r.nb = min(FA_TB, ntok - r.b0); r.pos0 = pos0; r.cache_off = 0;
    }
    return r;
}
// ---- pieces the three one-launch kernels share
// K / V tile staging: a 64-row tile travels global -> registers -> LDS, the next tile's loads in flight while the current one is consumed (clamped
// rows: every address is inside the cache, the surplus rows are never read).  8 float4 per thread cover a tile (host check).  The registers are the
// calling kernel's NAMED pk0..pk7 and the code stays a macro: a register array captured by a lambda, or filled in a macro loop, ends up in scratch
// with this compiler.  In scope: pk0..pk7, H4, HS, PITCH, kv_dim, kvh.
//   FA_FETCH(SRC_, TI_, TS_, T0_, ROWS_)   thread TI_ of TS_ loads its slots of the ROWS_ rows from timestep T0_ of the cache SRC_ (kc / vc)
//   FA_PARK(DST_, TI_, TS_)                the same slots -> the LDS tile DST_ ([64][PITCH])
#define FA_REP8(X_, ...) X_(0, __VA_ARGS__) X_(1, __VA_ARGS__) X_(2, __VA_ARGS__) X_(3, __VA_ARGS__) X_(4, __VA_ARGS__) X_(5, __VA_ARGS__) X_(6, __VA_ARGS__) X_(7, __VA_ARGS__)
#define FA_F(U_, SRC_, TI_, TS_, T0_, ROWS_) { const int fi = min((TI_) + U_ * (TS_), 64 * H4 - 1), fr = min(fi / H4, (ROWS_) - 1), fc = fi % H4; \
        pk##U_ = *reinterpret_cast<const float4*>((SRC_) + (size_t)((T0_) + fr) * kv_dim + kvh * HS + 4 * fc); }
#define FA_P(U_, DST_, TI_, TS_) { const int fi = (TI_) + U_ * (TS_); if (fi < 64 * H4) *reinterpret_cast<float4*>((DST_) + (fi / H4) * PITCH + 4 * (fi % H4)) = pk##U_; }
#define FA_FETCH(SRC_, TI_, TS_, T0_, ROWS_) do { const int ft0_ = (T0_), frows_ = (ROWS_); FA_REP8(FA_F, SRC_, TI_, TS_, ft0_, frows_) } while (0)
#define FA_PARK(DST_, TI_, TS_) do { FA_REP8(FA_P, DST_, TI_, TS_) } while (0)

// Phase 2, softmax of the tile's kvmul * nb score rows in LDS (FloatTensor.softmaxInPlace: max, exp in double, sequential f32 sum, divide).  Row
// (head hq, token tb) sits at Ssc + (hq * FA_TB + tb) * sstride and has pos0 + b0 + tb + 1 elements; its index here is hq * nb + tb.
// FA_SOFTMAX_NUMERATORS: every wavefront takes rows (max, e = exp), then lane = row of wavefront 0 runs the strictly sequential sums side by side
// (32 chains instead of one row per wavefront; reads pinned three groups ahead, gl3_decode_kernels.h) into sums[row].  Ends behind a barrier.
// In scope: Ssc, sums, sstride, nrows = kvmul * nb, nwaves, nb, pos0, b0, tmax, wave, lane.
#define FA_SOFTMAX_NUMERATORS() do { \
    for (int row = wave; row < nrows; row += nwaves) { \
        const int tb = row % nb, n = pos0 + b0 + tb + 1; \
        float* e = Ssc + (size_t)((row / nb) * FA_TB + tb) * sstride; \
        float mx = -INFINITY; \
        for (int i = lane; i < n; i += 64) mx = fmaxf(mx, e[i]); \
        mx = wave_max(mx); \
        for (int i = lane; i < n; i += 64) e[i] = (float)exp((double)(e[i] - mx)); \
    } \
    __syncthreads(); \
    if (wave == 0 && lane < nrows) { \
        const int tb = lane % nb, n = pos0 + b0 + tb + 1; \
        const float* e = Ssc + (size_t)((lane / nb) * FA_TB + tb) * sstride; \
        sums[lane] = seq_sum_lds_ring(e, n); \
    } \
    __syncthreads(); \
} while (0)
// FA_SOFTMAX_DIVIDE: e / sum in place.  ZERO_BEHIND (a phase 3 that masks by weight): weight 0 behind the token's position, up to where the
// wavefront that carries this token can read — its last token sits at most 3 positions further, rounded up to a group of four, inside the
// tile's last 64-timestep block.
#define FA_SOFTMAX_DIVIDE(ZERO_BEHIND) do { \
    for (int row = wave; row < nrows; row += nwaves) { \
        const int tb = row % nb, n = pos0 + b0 + tb + 1; \
        float* e = Ssc + (size_t)((row / nb) * FA_TB + tb) * sstride; \
        const float sum = sums[row]; \
        if (ZERO_BEHIND) { \
            const int zend = min((n + 4 + 63) & ~63, (tmax + 1 + 63) & ~63); \
            for (int i = lane; i < zend; i += 64) e[i] = i < n ? e[i] / sum : 0.f; \
        } else { \
            for (int i = lane; i < n; i += 64) e[i] = e[i] / sum; \
        } \
    } \
} while (0)

// The int8 output epilogues (r6): the attention output leaves the kernel as the wo projection's operand (int8 chunks XQ3[k / 16][token slot][16 B] +
// the scale-operand table of gl3_prefill_gemm3.h) instead of f32 + a quantise launch.
// Q8_ROUND_PAIR: declares Q0_, Q1_ = the Q8_0 codes (as bytes) of two values of a block whose largest magnitude is AMAX_, QS_ = the block scale before its f16 rounding
// (Q8_0FloatTensor.java:96-118 arithmetic as quantize_quad_pack).  The maximum over the block's lanes is the caller's: it depends on the lane layout.
#define Q8_ROUND_PAIR(AMAX_, V0_, V1_, QS_, Q0_, Q1_) \
    const float QS_ = (AMAX_) / 127.0f; \
    const float ainv = QS_ != 0.f ? 1.0f / QS_ : 0.f; \
    const float s0 = (V0_) * ainv, s1 = (V1_) * ainv; \
    const uint32_t Q0_ = (uint32_t)((int)(s0 + copysignf(0.5f, s0)) & 0xFF), Q1_ = (uint32_t)((int)(s1 + copysignf(0.5f, s1)) & 0xFF)
// FA_STORE_ROWS4: the output of the VALU kernels' phase 3 — the wavefront's four tokens 4 grp .. 4 grp + 3 of its head, lane = columns 2 lane, 2 lane + 1
// (head size 128) or column lane.  Quantised (head size 128, xq_out): a 32-element block of a token's row = 32 consecutive columns = the 16 lanes
// of a DPP row, two ADJACENT columns each.  In scope: acc[4][NCOL], grp, nb, b0, head, hreal (false: the
// surplus head slot of a ragged head group, which stores nothing), lane, out, out_stride, xq_out, xp_out, xp_tok.
#define FA_STORE_ROWS4() do { \
    if (NCOL == 2 && xq_out) { \
        _Pragma("unroll") for (int u = 0; u < 4; ++u) { \
            const int tb = 4 * grp + u; \
            float amax = fmaxf(fabsf(acc[u][0]), fabsf(acc[u][NCOL - 1])); \
            _Pragma("unroll") for (int m = 1; m < 16; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64)); \
            Q8_ROUND_PAIR(amax, acc[u][0], acc[u][NCOL - 1], qs, q0, q1); \
            if (tb >= nb || !hreal) continue; \
            const int col = head * HS + 2 * lane, b = b0 + tb; \
            *reinterpret_cast<uint16_t*>(xq_out + ((size_t)(col >> 4) * xp_tok + b) * 16 + (col & 15)) = (uint16_t)(q0 | (q1 << 8)); \
            if ((lane & 15) == 0) { \
                const G3ScaleOperands so = g3_scale_operands((float)(_Float16)qs); \
                const int blk = col >> 5; \
                xp_out[((size_t)blk * 2 + 0) * xp_tok + b] = so.half0; \
                xp_out[((size_t)blk * 2 + 1) * xp_tok + b] = so.half1; \
            } \
        } \
        return; \
    } \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) { \
        const int tb = 4 * grp + u; \
        if (tb >= nb || !hreal) continue; \
        _Pragma("unroll") for (int c = 0; c < NCOL; ++c) { \
            const int j = NCOL == 2 ? 2 * lane + c : lane; \
            if (j < HS) out[(size_t)(b0 + tb) * out_stride + head * HS + j] = acc[u][c]; \
        } \
    } } while (0)

template <int HS>
__global__ __launch_bounds__(512) void pf_attn_fused_kernel(const float* __restrict__ Q, int q_stride, const float* __restrict__ kc, const float* __restrict__ vc,
                                                            float* __restrict__ out, int out_stride, int n_kv_heads, int kvmul, int kv_dim,
                                                            int pos0, int ntok, float att_mul, int sstride,
                                                            uint8_t* __restrict__ xq_out = nullptr, uint4* __restrict__ xp_out = nullptr, int xp_tok = 0) {
    extern __shared__ __attribute__((aligned(16))) float fa_sm[];
    constexpr int PITCH = HS + 4, H4 = HS / 4, NCOL = HS > 64 ? 2 : 1;
    float* Ssc = fa_sm;                                             // [kvmul][FA_TB][sstride] score -> softmax rows
    float* kt = fa_sm + (size_t)kvmul * FA_TB * sstride;            // [2][64][PITCH] K (phase 1) / V (phase 3) tiles
    float* sums = kt + 2 * 64 * PITCH;                              // [kvmul * FA_TB]
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nthr = blockDim.x, gthreads = 64 * kvmul;
    const int grp = wave / kvmul, hq = wave % kvmul, gt = t - grp * gthreads;
    const int ntile = (ntok + FA_TB - 1) / FA_TB;
    const int kvh = blockIdx.x % n_kv_heads, tile = ntile - 1 - blockIdx.x / n_kv_heads;
    const int b0 = tile * FA_TB, nb = min(FA_TB, ntok - b0), tmax = pos0 + b0 + nb - 1;
    const int head = kvh * kvmul + hq;
    constexpr bool hreal = true;                                    // no head groups here: every wavefront's head is its own
    const float sqrt_hs = (float)sqrt((double)HS);

#ifdef FA_TIMING
    unsigned long long fa_t0 = __builtin_readcyclecounter(), fa_t1, fa_t2, fa_t3;
#endif
    // ---- phase 1: scores
    const int nkt = tmax / 64 + 1;
    float4 pk0, pk1, pk2, pk3, pk4, pk5, pk6, pk7;           // the staging registers of FA_FETCH / FA_PARK
    FA_FETCH(kc, gt, gthreads, min(grp * 64, tmax), max(1, min(64, tmax + 1 - grp * 64)));
    for (int trip = 0; 2 * trip < nkt; ++trip) {
        const int t0 = (2 * trip + grp) * 64;
        const bool live = t0 <= tmax;
        const int t1 = min(tmax + 1, t0 + 64);
        float* ktg = kt + grp * 64 * PITCH;
        if (live) FA_PARK(ktg, gt, gthreads);
        __syncthreads();
        FA_FETCH(kc, gt, gthreads, min(t0 + 128, tmax), max(1, min(64, tmax + 1 - (t0 + 128))));      // this group's next tile (clamped: fetched even if it is not used)
        if (live) {
            float4 kr[H4];
#pragma unroll
            for (int c = 0; c < H4; ++c) kr[c] = *reinterpret_cast<const float4*>(ktg + min(lane, t1 - t0 - 1) * PITCH + 4 * c);
            for (int tb = 0; tb < nb; tb += 2) {
                // the two query rows are wavefront-uniform: scalar loads, SGPR operands in the multiplies (as pf_scores_tiled_kernel)
                const float* q0 = Q + (size_t)(b0 + tb) * q_stride + (size_t)head * HS;
                const float* q1 = Q + (size_t)(b0 + min(tb + 1, nb - 1)) * q_stride + (size_t)head * HS;
                float s0 = 0.f, s1 = 0.f;
                if constexpr (HS >= 64) {
                    v16f_t a0, a1, c0, c1;
                    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %3, 0x0" : "=&s"(a0), "=&s"(a1) : "s"(q0), "s"(q1));
                    static_for<0, H4 / 4, 2>([&](auto ic) {
                        constexpr int c4 = decltype(ic)::value;
                        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+v"(s0), "+v"(s1));
                        asm volatile("s_load_dwordx16 %0, %2, %4\n\ts_load_dwordx16 %1, %3, %4" : "=&s"(c0), "=&s"(c1) : "s"(q0), "s"(q1), "n"((c4 + 1) * 64));
                        score_step16(s0, s1, a0, a1, &kr[4 * c4]);
                        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(c0), "+s"(c1), "+v"(s0), "+v"(s1));
                        if constexpr (c4 + 2 < H4 / 4)
                            asm volatile("s_load_dwordx16 %0, %2, %4\n\ts_load_dwordx16 %1, %3, %4" : "=&s"(a0), "=&s"(a1) : "s"(q0), "s"(q1), "n"((c4 + 2) * 64));
                        score_step16(s0, s1, c0, c1, &kr[4 * c4 + 4]);
                    });
                } else {
                    v16f_t a0, a1, c0, c1;
                    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %3, 0x0" : "=&s"(a0), "=&s"(a1) : "s"(q0), "s"(q1));
                    asm volatile("s_load_dwordx16 %0, %2, 64\n\ts_load_dwordx16 %1, %3, 64" : "=&s"(c0), "=&s"(c1) : "s"(q0), "s"(q1));
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+s"(c0), "+s"(c1), "+v"(s0), "+v"(s1));
                    score_step16(s0, s1, a0, a1, &kr[0]);
                    score_step16(s0, s1, c0, c1, &kr[4]);
                }
                const int ts = t0 + lane;
                if (ts < t1) {
                    if (ts <= pos0 + b0 + tb) Ssc[(size_t)(hq * FA_TB + tb) * sstride + ts] = att_mul != 0.f ? s0 * att_mul : s0 / sqrt_hs;
                    if (tb + 1 < nb && ts <= pos0 + b0 + tb + 1) Ssc[(size_t)(hq * FA_TB + tb + 1) * sstride + ts] = att_mul != 0.f ? s1 * att_mul : s1 / sqrt_hs;
                }
            }
        }
        __syncthreads();
    }

#ifdef FA_TIMING
    fa_t1 = __builtin_readcyclecounter();
#endif
    // the first V tile travels while the softmax runs
    FA_FETCH(vc, t, nthr, 0, min(64, tmax + 1));
    // ---- phase 2: softmax of the kvmul * nb rows
    const int nrows = kvmul * nb, nwaves = nthr >> 6;
    FA_SOFTMAX_NUMERATORS();
    FA_SOFTMAX_DIVIDE(false);

#ifdef FA_TIMING
    fa_t2 = __builtin_readcyclecounter();
#endif
    // ---- phase 3: weighted V sum; wavefront = (query head hq, tokens 4 * grp .. + 3)
    int posu[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) posu[u] = 4 * grp + u < nb ? pos0 + b0 + 4 * grp + u : -1;       // -1: no timestep qualifies
    const int wmax = 4 * grp < nb ? pos0 + b0 + min(4 * grp + 3, nb - 1) : -1;
    const float* as = Ssc + (size_t)(hq * FA_TB + 4 * grp) * sstride;                             // rows of this wavefront's four tokens
    float acc[4][NCOL];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < NCOL; ++c) acc[u][c] = 0.f;
    int vb = 0;
    for (int t0 = 0; t0 <= tmax; t0 += 64, vb ^= 1) {
        const int tt = min(64, tmax + 1 - t0);
        float* vt = kt + vb * 64 * PITCH;
        FA_PARK(vt, t, nthr);
        __syncthreads();                                             // (also orders phase 2's writes before the first reads of `as`)
        FA_FETCH(vc, t, nthr, min(t0 + 64, tmax), max(1, min(64, tmax + 1 - (t0 + 64))));
        const int ttw = min(tt, wmax + 1 - t0);
        const int rfull = (4 * grp + 3 < nb) ? max(0, min(tt, posu[0] + 1 - t0)) & ~3 : 0;       // timesteps all four tokens attend to
        auto vload = [&](int r, float (&v)[NCOL]) {
            if (NCOL == 2) {
                const float2 v2 = *reinterpret_cast<const float2*>(vt + r * PITCH + 2 * lane);
                v[0] = v2.x; v[NCOL - 1] = v2.y;
            } else {
                v[0] = lane < HS ? vt[r * PITCH + lane] : 0.f;
            }
        };
        // four timesteps per group; the next group's softmax weights and V rows are read from LDS while the current group is
        // accumulated (two named register sets: the un-pipelined loop spent ~2/3 of its time waiting for LDS, in-kernel stamps)
#define FA_LD(A_, V_, R_)                                                                                                    \
        do {                                                                                                                 \
            _Pragma("unroll") for (int u = 0; u < 4; ++u) A_[u] = *reinterpret_cast<const float4*>(as + (size_t)u * sstride + t0 + (R_)); \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) vload((R_) + i, V_[i]);                                             \
        } while (0)
#define FA_ACC(A_, V_)                                                                                                       \
        do {                                                                                                                 \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                    \
                _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                              \
                    const float at = i == 0 ? A_[u].x : i == 1 ? A_[u].y : i == 2 ? A_[u].z : A_[u].w;                        \
                    _Pragma("unroll") for (int c = 0; c < NCOL; ++c) acc[u][c] = at * V_[i][c] + acc[u][c];                   \
                }                                                                                                            \
        } while (0)
        float4 aA[4], aB[4];
        float vA[4][NCOL], vB[4][NCOL];
        if (rfull > 0) FA_LD(aA, vA, 0);
        int r = 0;
        for (; r + 8 <= rfull; r += 8) {
            FA_LD(aB, vB, r + 4);
            FA_ACC(aA, vA);
            if (r + 8 < rfull) FA_LD(aA, vA, r + 8);
            FA_ACC(aB, vB);
        }
        if (r < rfull) FA_ACC(aA, vA);                               // rfull is a multiple of 4: one group left
#undef FA_LD
#undef FA_ACC
        for (int r = rfull; r < ttw; ++r) {                          // the diagonal: per-token conditions (uniform)
            float v[NCOL];
            vload(r, v);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (t0 + r <= posu[u]) {
                    const float at = as[(size_t)u * sstride + t0 + r];
#pragma unroll
                    for (int c = 0; c < NCOL; ++c) acc[u][c] = at * v[c] + acc[u][c];
                }
            }
        }
    }
#ifdef FA_TIMING
    fa_t3 = __builtin_readcyclecounter();
    if (lane == 0 && kvh == 0 && (tile % 9) == 0) printf("fa tile %d wave %d: scores %llu softmax %llu pv %llu\n", tile, wave, fa_t1 - fa_t0, fa_t2 - fa_t1, fa_t3 - fa_t2);
#endif
    FA_STORE_ROWS4();
}

// r6 — pf_attn_fused_kernel with the inner loops of pf_scores_pk_kernel (phase 1: query rows interleaved in LDS, two tokens' chains per register pair
// on packed f32, reads of the next 8 steps pinned under the current group) and pf_pv_ring_kernel (phase 3: masking by zero weights, the next
// timestep group's LDS reads pinned under the current group's arithmetic).  Same arithmetic in the same order; 16 KB more LDS (query rows).
// kvmul = head slots of the workgroup (the head group's size: min(kvMul, 4)), kvm = the model's kvMul, which indexes the heads.
__host__ __device__ constexpr size_t fa2_smem_bytes(int hs, int kvmul, int sstride) { return fa_smem_bytes(hs, kvmul, sstride) + (size_t)kvmul * FA_TB * hs * 4; }
template <int HS, bool TAB = false>
__global__ __launch_bounds__(512) void pf_attn_fused2_kernel(const float* __restrict__ Q, int q_stride, const float* __restrict__ kc, const float* __restrict__ vc,
                                                            float* __restrict__ out, int out_stride, int n_kv_heads, int kvmul, int kvm, int kv_dim,
                                                            int pos0, int ntok, float att_mul, int sstride,
                                                            uint8_t* __restrict__ xq_out = nullptr, uint4* __restrict__ xp_out = nullptr, int xp_tok = 0,
                                                            const int4* __restrict__ tab = nullptr, size_t seq_stride = 0) {
    extern __shared__ __attribute__((aligned(16))) float fa_sm[];
    constexpr int PITCH = HS + 4, H4 = HS / 4, NCOL = HS > 64 ? 2 : 1;
    float* Ssc = fa_sm;                                             // [kvmul][FA_TB][sstride] score -> softmax rows
    float* kt = fa_sm + (size_t)kvmul * FA_TB * sstride;            // [2][64][PITCH] K (phase 1) / V (phase 3) tiles
    float* sums = kt + 2 * 64 * PITCH;                              // [kvmul * FA_TB] (+ padding to 64 floats)
    float* qs = sums + 64;                                          // [kvmul][FA_TB / 2 pairs][HS][2] query rows, interleaved by token pairs
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nthr = blockDim.x, gthreads = 64 * kvmul;
    const int grp = wave / kvmul, hq = wave % kvmul, gt = t - grp * gthreads;
    const FaTile ft = fa_tile<TAB>(n_kv_heads, pos0, ntok, tab, seq_stride);
    const HeadGroup hg = head_group(ft.kvh, ft.g, kvm, kvmul);
    const int kvh = ft.kvh, b0 = ft.b0, nb = ft.nb;
    pos0 = ft.pos0; kc += ft.cache_off; vc += ft.cache_off;      // of the tile's sequence from here on
    const int tmax = pos0 + b0 + nb - 1;
    const int head = hg.head_of(hq);
    const bool hreal = hg.real(hq);
    const float sqrt_hs = (float)sqrt((double)HS);

#ifdef FA_TIMING
    unsigned long long fa_t0 = __builtin_readcyclecounter(), fa_t1, fa_t2, fa_t3;
#endif
    // ---- phase 1: scores
    const int nkt = tmax / 64 + 1;
    float4 pk0, pk1, pk2, pk3, pk4, pk5, pk6, pk7;           // the staging registers of FA_FETCH / FA_PARK
    FA_FETCH(kc, gt, gthreads, min(grp * 64, tmax), max(1, min(64, tmax + 1 - grp * 64)));
    // query rows of the tile's tokens -> LDS, interleaved by token pairs: {q_a[j], q_b[j], q_a[j + 1], q_b[j + 1]} is one 16-byte broadcast read
    for (int i = t; i < kvmul * (FA_TB / 2) * H4; i += nthr) {
        const int c = i % H4, pair = (i / H4) % (FA_TB / 2), qh = i / (H4 * (FA_TB / 2));
        const float* qp = Q + (size_t)hg.head_of(qh) * HS + 4 * c;
        const v4f_native_s xa = *reinterpret_cast<const v4f_native_s*>(qp + (size_t)(b0 + min(2 * pair, nb - 1)) * q_stride);
        const v4f_native_s xb = *reinterpret_cast<const v4f_native_s*>(qp + (size_t)(b0 + min(2 * pair + 1, nb - 1)) * q_stride);
        float* d = qs + ((size_t)(qh * (FA_TB / 2) + pair) * HS + 4 * c) * 2;
        *reinterpret_cast<v4f_native_s*>(d) = (v4f_native_s){xa.x, xb.x, xa.y, xb.y};
        *reinterpret_cast<v4f_native_s*>(d + 4) = (v4f_native_s){xa.z, xb.z, xa.w, xb.w};
    }
    for (int trip = 0; 2 * trip < nkt; ++trip) {
        const int t0 = (2 * trip + grp) * 64;
        const bool live = t0 <= tmax;
        const int t1 = min(tmax + 1, t0 + 64);
        float* ktg = kt + grp * 64 * PITCH;
        if (live) FA_PARK(ktg, gt, gthreads);
        __syncthreads();
        FA_FETCH(kc, gt, gthreads, min(t0 + 128, tmax), max(1, min(64, tmax + 1 - (t0 + 128))));      // this group's next tile (clamped: fetched even if it is not used)
        if (live) {
            v2f_native kr[HS / 2];
#pragma unroll
            for (int c = 0; c < H4; ++c) {
                const v4f_native_s x = *reinterpret_cast<const v4f_native_s*>(ktg + min(lane, t1 - t0 - 1) * PITCH + 4 * c);
                kr[2 * c] = x.xy; kr[2 * c + 1] = x.zw;
            }
            for (int pp = 0; 4 * pp < nb; ++pp) {                    // four tokens = two packed chains per pass (pf_scores_pk_kernel's inner loop)
                const float* q01 = qs + (size_t)(hq * (FA_TB / 2) + 2 * pp) * HS * 2;
                const float* q23 = q01 + HS * 2;
                v2f_native c0 = {0.f, 0.f}, c1 = {0.f, 0.f};
                v4f_native_s qa[8], qb[8];
                SPK_LD(0, qa); SPK_LD(1, qb); __builtin_amdgcn_sched_barrier(0);
                static_for<0, HS / 8, 2>([&](auto gc) {
                    constexpr int g = decltype(gc)::value;
                    SPK_ACC(g, qa);
                    SPK_LD((g + 2 < HS / 8 ? g + 2 : HS / 8 - 1), qa); __builtin_amdgcn_sched_barrier(0);
                    SPK_ACC(g + 1, qb);
                    SPK_LD((g + 3 < HS / 8 ? g + 3 : HS / 8 - 1), qb); __builtin_amdgcn_sched_barrier(0);
                });
                const float sv[4] = {c0.x, c0.y, c1.x, c1.y};
                const int ts = t0 + lane;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int tb = 4 * pp + u;
                    if (tb < nb && ts <= pos0 + b0 + tb) Ssc[(size_t)(hq * FA_TB + tb) * sstride + ts] = att_mul != 0.f ? sv[u] * att_mul : sv[u] / sqrt_hs;
                }
            }
        }
        __syncthreads();
    }

#ifdef FA_TIMING
    fa_t1 = __builtin_readcyclecounter();
#endif
    // the first V tile travels while the softmax runs
    FA_FETCH(vc, t, nthr, 0, min(64, tmax + 1));
    // ---- phase 2: softmax of the kvmul * nb rows
    const int nrows = kvmul * nb, nwaves = nthr >> 6;
    FA_SOFTMAX_NUMERATORS();
    FA_SOFTMAX_DIVIDE(true);

#ifdef FA_TIMING
    fa_t2 = __builtin_readcyclecounter();
#endif
    // ---- phase 3: weighted V sum; wavefront = (query head hq, tokens 4 * grp .. + 3)
    const int wmax = 4 * grp < nb ? pos0 + b0 + min(4 * grp + 3, nb - 1) : -1;
    const float* as = Ssc + (size_t)(hq * FA_TB + 4 * grp) * sstride;                             // rows of this wavefront's four tokens
    float acc[4][NCOL];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < NCOL; ++c) acc[u][c] = 0.f;
    int vb = 0;
    for (int t0 = 0; t0 <= tmax; t0 += 64, vb ^= 1) {
        const int tt = min(64, tmax + 1 - t0);
        float* vt = kt + vb * 64 * PITCH;
        FA_PARK(vt, t, nthr);
        __syncthreads();                                             // (also orders phase 2's writes before the first reads of `as`)
        FA_FETCH(vc, t, nthr, min(t0 + 64, tmax), max(1, min(64, tmax + 1 - (t0 + 64))));
        // groups of four timesteps; the next group's weights and V rows are read from LDS under the current group's arithmetic (pinned).
        // Timesteps behind a token's position carry the weight 0 (0 * v + acc = acc exactly; every staged V row is a written row).
        const int ng = max(0, min(64, wmax + 1 - t0) + 3) >> 2;
        const float* ap = as + t0;
        const float* vp = vt + (NCOL == 2 ? 2 * lane : min(lane, HS - 1));
        PVR_TILE(ng, sstride, PITCH);
    }
#ifdef FA_TIMING
    fa_t3 = __builtin_readcyclecounter();
    if (lane == 0 && kvh == 0 && (b0 % 72) == 0) printf("fa tile %d wave %d: scores %llu softmax %llu pv %llu\n", b0 / FA_TB, wave, fa_t1 - fa_t0, fa_t2 - fa_t1, fa_t3 - fa_t2);
#endif
    FA_STORE_ROWS4();
}


// r6 — the one-launch prefill attention with the PRODUCTS of phases 1 and 3 on the matrix pipe (a head group of 4 slots — kvMul 4, or kvm >= 5
// in groups, HeadGroup above: 32 (head slot, token) rows per workgroup).
// pf_attn_fused_kernel / fused2 feed one operand of every multiply from a wavefront-uniform place (SGPRs: lead bounded by the SGPR file; LDS:
// a uniform-address ds_read_b128 costs 9.2 cycles of the CU's LDS pipe against 4.9 for 64 distinct addresses, scripts/probes/lds_bcast_probe.hip)
// and both phases end up bound by that delivery.  A K = 1 f32 MFMA with C = 0 is an outer product of two LANE-DISTINCT vectors whose every
// element is rounded once (D = fma(a, b, 0) = fl(a * b): the property gemm_vlq_mfma_kernel uses): v_mfma_f32_16x16x1_4b_f32 = four independent
// 16 x 16 blocks per instruction, 1024 rounded products in 32 cycles, no broadcast anywhere; the VALU keeps the ordered adds (packed).
//   phase 1  wavefront = 16 timesteps of the K tile x all 32 rows.  Block q = (row group q & 1, step parity q >> 1): A = k[t][2 m + parity]
//            (the lane's K row, every second element, in registers), B = q[row][2 m + parity] (one ds_read_b32 of 64 distinct addresses).
//            Per MFMA the chains advance two steps: s = (s + P_even) + P_odd, j ascending.  64 MFMAs + 512 packed adds per tile and wavefront.
//   phase 3  wavefront = 16 rows x 32 columns.  Block q = (column group q & 1, timestep parity q >> 1): A = w[row][t + parity] (softmax weight,
//            0 behind the row's position), B = v[t + parity][column]; acc = (acc + P_t) + P_t+1, t ascending.  8 accumulator registers.
// Same arithmetic, same order, same roundings as InferenceCore.java:98-137; phase 2 is pf_attn_fused_kernel's.
__host__ __device__ constexpr size_t fa3_smem_bytes(int hs, int sstride) {
    return ((size_t)4 * FA_TB * sstride + 2 * 64 * (hs + 4) + 64 + (size_t)4 * FA_TB * (hs + 2)) * 4;
}
// ---- the MFMA chains (pf_attn_fused3_kernel, pf_scores_mfma_kernel, pf_pv_mfma_kernel)
// F3_SCORE_TILE(KROW_): the lane's K row KROW_ against 32 query rows, HS steps; sc[0..3] / sc[4..7] = the chains of the lane's two row groups at
// four timesteps.  In scope: sc (v8f_native), qrow (the lane's query row in LDS, + step parity), par, zero16, H4, NM = HS / 2.
#define F3_LDQ(G_, R_) do { _Pragma("unroll") for (int u_ = 0; u_ < 8; ++u_) R_[u_] = qrow[2 * (8 * (G_) + u_)]; } while (0)
// blocks 0 / 1 = row groups 0 / 1 at the even step, blocks 2 / 3 at the odd step: two dependent adds per chain and MFMA
#define F3_ADD(P_, S_) do { S_ = S_ + __builtin_shufflevector(P_, P_, 0, 1, 2, 3, 4, 5, 6, 7); S_ = S_ + __builtin_shufflevector(P_, P_, 8, 9, 10, 11, 12, 13, 14, 15); } while (0)
// one MFMA ahead of the adds that consume the previous one (two product registers, order pinned: left alone the scheduler issues a whole group's
// MFMAs first and spills their 8 x 16 result registers; every element's adds stay with their MFMA: left alone the chains are scalarised,
// re-vectorised pair by pair and the products spilled).  PIN_: a statement between the MFMA and the adds (fused3 pins there too).
#define F3_MF8(G_, R_, RN_, PIN_) do { _Pragma("unroll") for (int u_ = 0; u_ < 8; ++u_) { \
                const int mn_ = 8 * (G_) + u_ + 1;      /* a constant after unrolling */ \
                v16f_t Pn_ = Pc; \
                if (mn_ < NM) Pn_ = __builtin_amdgcn_mfma_f32_16x16x1f32(kreg[mn_ < NM ? mn_ : 0], u_ < 7 ? R_[u_ < 7 ? u_ + 1 : 0] : RN_[0], zero16, 0, 0, 0); \
                PIN_; \
                F3_ADD(Pc, sc); asm volatile("" : "+v"(sc)); \
                __builtin_amdgcn_sched_barrier(0); \
                Pc = Pn_; } } while (0)
#define F3_SCORE_TILE(KROW_, PIN_) do { \
            float kreg[NM];                                          /* k[t][2 m + parity], m ascending */ \
            _Pragma("unroll") for (int c = 0; c < H4; ++c) { \
                const v4f_native_s x = *reinterpret_cast<const v4f_native_s*>((KROW_) + 4 * c); \
                kreg[2 * c] = par ? x.y : x.x; kreg[2 * c + 1] = par ? x.w : x.z; \
            } \
            float qa[8], qb[8]; \
            F3_LDQ(0, qa); F3_LDQ(1, qb); __builtin_amdgcn_sched_barrier(0); \
            v16f_t Pc = __builtin_amdgcn_mfma_f32_16x16x1f32(kreg[0], qa[0], zero16, 0, 0, 0); \
            static_for<0, NM / 8, 2>([&](auto gc) { \
                constexpr int g = decltype(gc)::value; \
                F3_MF8(g, qa, qb, PIN_); \
                F3_LDQ((g + 2 < NM / 8 ? g + 2 : NM / 8 - 1), qa); __builtin_amdgcn_sched_barrier(0); \
                F3_MF8(g + 1, qb, qa, PIN_); \
                F3_LDQ((g + 3 < NM / 8 ? g + 3 : NM / 8 - 1), qb); __builtin_amdgcn_sched_barrier(0); \
            }); } while (0)
// F3_PV_TILE(NGR_): 16 rows x 32 columns advance through one 64-timestep V tile, NGR_ groups of 8 MFMAs = 16 timesteps each (a group past the tile's
// last attended pair multiplies zero weights: exact, acc + 0).  In scope: ac (v8f_native), wp (the lane's weight row at the tile's first timestep,
// + parity), vp (the lane's column of the tile's first V row, + parity rows), PITCH, zero16.
#define F3_LDV(G_, W_, V_) do { _Pragma("unroll") for (int u_ = 0; u_ < 8; ++u_) { const int m_ = min(8 * (G_) + u_, 31); W_[u_] = wp[2 * m_]; V_[u_] = vp[2 * m_ * PITCH]; } } while (0)
#define F3_PV8(W_, V_) do { v16f_t Pc_ = __builtin_amdgcn_mfma_f32_16x16x1f32(W_[0], V_[0], zero16, 0, 0, 0); \
                _Pragma("unroll") for (int u_ = 0; u_ < 8; ++u_) { \
                    v16f_t Pn_ = Pc_; \
                    if (u_ < 7) Pn_ = __builtin_amdgcn_mfma_f32_16x16x1f32(W_[u_ < 7 ? u_ + 1 : 0], V_[u_ < 7 ? u_ + 1 : 0], zero16, 0, 0, 0); \
                    __builtin_amdgcn_sched_barrier(0); \
                    F3_ADD(Pc_, ac); asm volatile("" : "+v"(ac)); \
                    __builtin_amdgcn_sched_barrier(0); \
                    Pc_ = Pn_; } } while (0)
#define F3_PV_TILE(NGR_) do { const int ngr_ = (NGR_); \
            float wa[8], va[8], wb[8], vb8[8]; \
            F3_LDV(0, wa, va); F3_LDV(1, wb, vb8); __builtin_amdgcn_sched_barrier(0); \
            int g = 0; \
            for (; g + 2 <= ngr_; g += 2) { \
                F3_PV8(wa, va); \
                F3_LDV(g + 2, wa, va); __builtin_amdgcn_sched_barrier(0); \
                F3_PV8(wb, vb8); \
                F3_LDV(g + 3, wb, vb8); __builtin_amdgcn_sched_barrier(0); \
            } \
            if (g < ngr_) F3_PV8(wa, va); } while (0)
template <int HS, bool TAB = false>
__global__ __launch_bounds__(512) void pf_attn_fused3_kernel(const float* __restrict__ Q, int q_stride, const float* __restrict__ kc, const float* __restrict__ vc,
                                                             float* __restrict__ out, int out_stride, int n_kv_heads, int kvm, int kv_dim,
                                                             int pos0, int ntok, float att_mul, int sstride,
                                                             uint8_t* __restrict__ xq_out, uint4* __restrict__ xp_out, int xp_tok,
                                                             const int4* __restrict__ tab = nullptr, size_t seq_stride = 0) {
    extern __shared__ __attribute__((aligned(16))) float fa_sm[];
    constexpr int KVM = 4, ROWS = KVM * FA_TB, PITCH = HS + 4, H4 = HS / 4, QP = HS + 2, NM = HS / 2, kvmul = KVM;
    static_assert(ROWS == 32 && NM % 16 == 0, "two row groups of 16; operand ring of 8 MFMAs");
    float* Ssc = fa_sm;                                             // [ROWS][sstride] score -> softmax rows, row = head * FA_TB + token
    float* kt = fa_sm + (size_t)ROWS * sstride;                     // [2][64][PITCH] K (phase 1) / V (phase 3) tiles
    float* sums = kt + 2 * 64 * PITCH;                              // [ROWS] (+ padding to 64 floats)
    float* qs = sums + 64;                                          // [ROWS][QP] query rows
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    constexpr int nthr = 512, gthreads = 256;
    const int grp = wave >> 2, wg = wave & 3, gt = t - grp * gthreads;
    const int lq = lane >> 4, li = lane & 15, par = lq >> 1;        // MFMA block of this lane's operands, index inside it, step parity of the block
    const FaTile ft = fa_tile<TAB>(n_kv_heads, pos0, ntok, tab, seq_stride);
    const HeadGroup hg = head_group(ft.kvh, ft.g, kvm, KVM);
    const int kvh = ft.kvh, b0 = ft.b0, nb = ft.nb;
    pos0 = ft.pos0; kc += ft.cache_off; vc += ft.cache_off;      // of the tile's sequence from here on
    const int tmax = pos0 + b0 + nb - 1;
    const float sqrt_hs = (float)sqrt((double)HS);
    const v16f_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int nkt = tmax / 64 + 1;
    float4 pk0, pk1, pk2, pk3, pk4, pk5, pk6, pk7;           // the staging registers of FA_FETCH / FA_PARK
    FA_FETCH(kc, gt, gthreads, min(grp * 64, tmax), max(1, min(64, tmax + 1 - grp * 64)));
    for (int i = t; i < ROWS * H4; i += nthr) {                      // query rows (tokens past the chunk's end repeat its last token: never stored)
        const int row = i / H4, c = i % H4;
        const float4 x = *reinterpret_cast<const float4*>(Q + (size_t)(b0 + min(row & (FA_TB - 1), nb - 1)) * q_stride + (size_t)hg.head_of(row >> 3) * HS + 4 * c);
        float* d = qs + row * QP + 4 * c;
        *reinterpret_cast<float2*>(d) = make_float2(x.x, x.y);
        *reinterpret_cast<float2*>(d + 2) = make_float2(x.z, x.w);
    }
#ifdef FA_TIMING
    unsigned long long fa_t0 = __builtin_readcyclecounter(), fa_t1, fa_t2, fa_t3;
#endif
    // ---- phase 1: scores
    for (int trip = 0; 2 * trip < nkt; ++trip) {
        const int t0 = (2 * trip + grp) * 64;
        const bool live = t0 <= tmax;
        const int t1 = min(tmax + 1, t0 + 64);
        float* ktg = kt + grp * 64 * PITCH;
        if (live) FA_PARK(ktg, gt, gthreads);
        __syncthreads();
        FA_FETCH(kc, gt, gthreads, min(t0 + 128, tmax), max(1, min(64, tmax + 1 - (t0 + 128))));      // this group's next tile (clamped: fetched even if it is not used)
        if (live && t0 + 16 * wg <= tmax) {                          // this wavefront's 16 timesteps hold at least one attended position
            const float* krow = ktg + min(16 * wg + li, t1 - t0 - 1) * PITCH;
            const float* qrow = qs + (16 * (lq & 1) + li) * QP + par;
            v8f_native sc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // [0..3] row li, [4..7] row 16 + li; the four timesteps 16 wg + 4 lq + r
            F3_SCORE_TILE(krow, __builtin_amdgcn_sched_barrier(0));
            // lane (lq, li) holds rows li and 16 + li at the timesteps 16 wg + 4 lq + r
            const float sv[2][4] = {{sc[0], sc[1], sc[2], sc[3]}, {sc[4], sc[5], sc[6], sc[7]}};
#pragma unroll
            for (int rgp = 0; rgp < 2; ++rgp) {
                const int row = 16 * rgp + li, tb = row & (FA_TB - 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ts = t0 + 16 * wg + 4 * lq + r;
                    if (tb < nb && ts <= pos0 + b0 + tb) Ssc[(size_t)row * sstride + ts] = att_mul != 0.f ? sv[rgp][r] * att_mul : sv[rgp][r] / sqrt_hs;
                }
            }
        }
        __syncthreads();
    }
#ifdef FA_TIMING
    fa_t1 = __builtin_readcyclecounter();
#endif
    // the first V tile travels while the softmax runs
    FA_FETCH(vc, t, nthr, 0, min(64, tmax + 1));
    // ---- phase 2: softmax of the kvmul * nb rows (pf_attn_fused_kernel's; weights behind a row's position are written as 0: phase 3 masks by weight)
    const int nrows = kvmul * nb, nwaves = nthr >> 6;
    FA_SOFTMAX_NUMERATORS();
    const int tend = (tmax + 1 + 63) & ~63;
    for (int row = wave; row < ROWS; row += nwaves) {                // every row of the tile: rows of tokens past the chunk's end become all-zero weights
        const int tb = row & (FA_TB - 1), hqr = row >> 3;
        float* e = Ssc + (size_t)row * sstride;
        const int n = tb < nb ? pos0 + b0 + tb + 1 : 0;
        const float sum = tb < nb ? sums[hqr * nb + tb] : 1.f;
        for (int i = lane; i < tend; i += 64) e[i] = i < n ? e[i] / sum : 0.f;
    }
#ifdef FA_TIMING
    fa_t2 = __builtin_readcyclecounter();
#endif
    // ---- phase 3: weighted V sum; wavefront = (row group rg, 32 columns cq)
    const int rg = wave & 1, cq = wave >> 1, cg = lq & 1;
    const bool pv_live = cq < HS / 32;
    v8f_native ac = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // [0..3] column 32 cq + li, [4..7] column 32 cq + 16 + li; rows 16 rg + 4 lq + r
    const float* wrow = Ssc + (size_t)(16 * rg + li) * sstride + par;
    int vb = 0;
    for (int t0 = 0; t0 <= tmax; t0 += 64, vb ^= 1) {
        float* vt = kt + vb * 64 * PITCH;
        FA_PARK(vt, t, nthr);
        __syncthreads();                                             // (also orders phase 2's writes before the first reads of the weights)
        FA_FETCH(vc, t, nthr, min(t0 + 64, tmax), max(1, min(64, tmax + 1 - (t0 + 64))));
        if (pv_live) {
            const int npair = (min(64, tmax + 1 - t0) + 1) >> 1;     // timestep pairs of the tile that hold an attended position (weights behind: 0)
            const float* wp = wrow + t0;
            const float* vp = vt + par * PITCH + 32 * cq + 16 * cg + li;
            F3_PV_TILE((npair + 7) >> 3);
        }
    }
#ifdef FA_TIMING
    fa_t3 = __builtin_readcyclecounter();
    if (lane == 0 && kvh == 0 && (b0 % 72) == 0) printf("fa tile %d wave %d: scores %llu softmax %llu pv %llu\n", b0 / FA_TB, wave, fa_t1 - fa_t0, fa_t2 - fa_t1, fa_t3 - fa_t2);
#endif
    if (!pv_live) return;
    const float av[2][4] = {{ac[0], ac[1], ac[2], ac[3]}, {ac[4], ac[5], ac[6], ac[7]}};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * rg + 4 * lq + r, tb = row & (FA_TB - 1), head = hg.h0 + (row >> 3), b = b0 + tb;
        const bool hreal = hg.real(row >> 3);                        // a surplus head slot of a ragged group stores nothing
        const int col = head * HS + 32 * cq + li;                    // av[0][r]; av[1][r] sits 16 columns further
        if (xq_out) {
            // quantised: this wavefront's 32 columns of a row are one Q8_0 block = the 16 lanes of a DPP row x 2 registers, columns 16 APART
            float amax = fmaxf(fabsf(av[0][r]), fabsf(av[1][r]));
            amax = row8_max(amax); GL3_DPP_MAX(amax, 0x140);
            Q8_ROUND_PAIR(amax, av[0][r], av[1][r], qsc, q0, q1);
            if (tb >= nb || !hreal) continue;
            xq_out[((size_t)(col >> 4) * xp_tok + b) * 16 + li] = (uint8_t)q0;
            xq_out[((size_t)((col >> 4) + 1) * xp_tok + b) * 16 + li] = (uint8_t)q1;
            if (li == 0) {
                const G3ScaleOperands so = g3_scale_operands((float)(_Float16)qsc);
                const int blk = col >> 5;
                xp_out[((size_t)blk * 2 + 0) * xp_tok + b] = so.half0;
                xp_out[((size_t)blk * 2 + 1) * xp_tok + b] = so.half1;
            }
        } else if (tb < nb && hreal) {
            out[(size_t)b * out_stride + col] = av[0][r];
            out[(size_t)b * out_stride + col + 16] = av[1][r];
        }
    }
}

// r6 — the weighted V sum behind a long context with its products on the matrix pipe (phase 3 of pf_attn_fused3_kernel as a kernel of its own; a head
// group of 4 slots).  Workgroup = (kv head and head group, 16 tokens) = four row groups (one per head slot) x HS / 32 column slices = 16 wavefronts; a wavefront advances its
// 16 rows x 32 columns two timesteps per MFMA: A = w[row][t + parity] (numerator / sum, 0 behind the row's position: staged that way), B = v[t + parity]
// [column], acc = (acc + P_t) + P_t+1.  Operands are lane-distinct 4-byte LDS reads (pf_pv_ring_kernel's uniform-address weight reads kept the
// LDS pipe 68 % busy and bound it).  Staging as pf_pv_ring_kernel: the next tile's V rows and numerators travel in registers under the current
// tile's arithmetic.
constexpr int PVM_TB = 16, PVM_WP = 68;
__host__ __device__ constexpr size_t pv_mfma_smem_bytes(int hs) { return ((size_t)64 * (hs + 4) + 4 * PVM_TB * PVM_WP) * 4; }
template <int HS, bool TAB = false>
__global__ __launch_bounds__(1024) void pf_pv_mfma_kernel(const PfAttnArgs a, int seq, int pos0, int ntok, const float* __restrict__ sums,
                                                          const int4* __restrict__ tab = nullptr) {
    constexpr int PITCH = HS + 4, H4 = HS / 4, NT = 1024, VPT = 64 * H4 / NT, KVM = 4;
    static_assert(VPT >= 1, "a V tile is at least one 16-byte slot per thread");
    extern __shared__ __attribute__((aligned(16))) float vt[];        // [64][PITCH] V rows, then [4 heads x 16 tokens][PVM_WP] weights
    float* ws = vt + 64 * PITCH;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int rg = wave & 3, cq = wave >> 2;                          // query head of the kv group, 32-column slice
    const int lq = lane >> 4, li = lane & 15, par = lq >> 1, cg = lq & 1;
    const LcTile lt = lc_tile<TAB, PVM_TB>(blockIdx.y, pos0, ntok, tab, a.seq_stride);
    const HeadGroup hg = lc_head_group(blockIdx.x, a.n_heads / a.n_kv_heads, KVM);
    const int kvh = hg.kvh, b0 = lt.b0, nb = lt.nb;
    pos0 = lt.pos0;
    const int tmax = pos0 + b0 + nb - 1, ntile = tmax / 64 + 1;
    const float* vc = a.vcache + (TAB ? lt.cache_off : (size_t)seq * a.seq_stride) + kvh * HS;
    const v16f_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // staging roles: thread = (row wave + 16 j, timestep lane) of the weights; 16-byte slots t + NT j of the V tile
    const float* arow[4]; float rsum[4]; int apos[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = wave + 16 * j, hq = row >> 4, tb = row & 15, b = b0 + min(tb, nb - 1);
        apos[j] = tb < nb ? pos0 + b0 + tb : -1;
        arow[j] = a.att + ((size_t)b * a.n_heads + hg.head_of(hq)) * a.ctx;
        rsum[j] = sums[(size_t)b * a.n_heads + hg.head_of(hq)];
    }
    typedef float v4f_native __attribute__((ext_vector_type(4)));
    v4f_native vreg[VPT]; float areg[4];
#define PVM_GLOAD(K_) do { const int t0_ = 64 * (K_); \
        static_for<0, VPT, 1>([&](auto jc) { constexpr int j = decltype(jc)::value; const int i = t + NT * j, r = i / H4, c = i % H4; \
            vreg[j] = *reinterpret_cast<const v4f_native*>(vc + (size_t)min(t0_ + r, tmax) * a.kv_dim + 4 * c); }); \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) areg[j] = arow[j][max(min(t0_ + lane, apos[j]), 0)]; } while (0)
#define PVM_LSTORE(K_) do { const int t0_ = 64 * (K_); \
        static_for<0, VPT, 1>([&](auto jc) { constexpr int j = decltype(jc)::value; const int i = t + NT * j, r = i / H4, c = i % H4; \
            *reinterpret_cast<v4f_native*>(vt + r * PITCH + 4 * c) = vreg[j]; }); \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) ws[(wave + 16 * j) * PVM_WP + lane] = t0_ + lane <= apos[j] ? areg[j] / rsum[j] : 0.f; } while (0)
    v8f_native ac = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};          // [0..3] column 32 cq + li, [4..7] column 32 cq + 16 + li; tokens 4 lq + r of head rg
    const bool live = cq < HS / 32 && hg.real(rg);                   // (a surplus head slot still stages and reaches every barrier)
    const float* wp = ws + (16 * rg + li) * PVM_WP + par;
    const float* vp = vt + par * PITCH + 32 * cq + 16 * cg + li;
    PVM_GLOAD(0);
    PVM_LSTORE(0);
    __syncthreads();
    for (int k = 0; k < ntile; ++k) {
        PVM_GLOAD(min(k + 1, ntile - 1));                            // unconditional (a condition around the loads makes the compiler drain them)
        if (live) {
            const int npair = (min(64, tmax + 1 - 64 * k) + 1) >> 1, ngr = (npair + 7) >> 3;
            F3_PV_TILE(ngr);
        }
        __syncthreads();
        PVM_LSTORE(min(k + 1, ntile - 1));
        __syncthreads();
    }
#undef PVM_GLOAD
#undef PVM_LSTORE
    if (!live) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int tb = 4 * lq + r;
        if (tb >= nb) continue;
        float* o = a.out + (size_t)(b0 + tb) * a.out_stride + (size_t)(hg.h0 + rg) * HS + 32 * cq + li;
        o[0] = ac[r]; o[16] = ac[4 + r];
    }
}

// r6 — the scores behind a long context with their products on the matrix pipe (phase 1 of pf_attn_fused3_kernel as a kernel of its own; a head group of 4 slots).
// Workgroup = (kv head, 16 tokens, every S-th K tile): 64 (head, token) rows whose query rows stay in LDS for the workgroup's whole life; 8 wavefronts
// = 4 quarters of a 64-timestep K tile x 2 pairs of row groups.  Block q of an MFMA = (row group of the pair q & 1, step parity q >> 1): A = k[t][2 m +
// parity] (the lane's K row, every second element, in registers), B = q[row][2 m + parity] (64 distinct LDS addresses); the chains advance two steps
// per MFMA, s = (s + P_even) + P_odd, j ascending.  The next K tile travels in registers under the current tile's arithmetic.  Per-tile row maxima
// for pf_softmax_rows_kernel: registers -> two cross-row exchanges -> one LDS slot per (quarter, row) -> 64 threads fold the quarters.
constexpr int SCM_TB = 16, SCM_SPLIT = 4;
__host__ __device__ constexpr size_t scores_mfma_smem_bytes(int hs) { return ((size_t)64 * (hs + 4) + 4 * SCM_TB * (hs + 2) + 4 * 4 * SCM_TB) * 4; }
template <int HS, bool TAB = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void pf_scores_mfma_kernel(const float* __restrict__ Q, int q_stride, const float* __restrict__ kc, float* __restrict__ att,
                                                             int n_heads, int kvm, int kv_dim, int ctx, int pos0, int ntok, float att_mul, float* __restrict__ tmx, int tmx_tiles,
                                                             const int4* __restrict__ tab = nullptr, size_t seq_stride = 0) {
    extern __shared__ __attribute__((aligned(16))) float kt[];       // [64][PITCH] K rows, then [64 rows][QP] query rows, then [4][64] quarter maxima
    constexpr int KVM = 4, ROWS = KVM * SCM_TB, PITCH = HS + 4, H4 = HS / 4, QP = HS + 2, NM = HS / 2, NT = 512, KPT = 64 * H4 / NT;
    static_assert(KPT >= 1 && NM % 16 == 0, "staging slots per thread; operand ring of 8 MFMAs");
    float* qs = kt + 64 * PITCH;
    float* mxs = qs + ROWS * QP;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tq = wave & 3, rp = wave >> 2;
    const int lq = lane >> 4, li = lane & 15, par = lq >> 1, rsel = lq & 1;
    const LcTile lt = lc_tile<TAB, SCM_TB>(blockIdx.z, pos0, ntok, tab, seq_stride);
    const HeadGroup hg = lc_head_group(blockIdx.y, kvm, KVM);
    const int split = blockIdx.x, nsplit = gridDim.x, kvh = hg.kvh, b0 = lt.b0, nb = lt.nb;
    pos0 = lt.pos0; kc += lt.cache_off;               // of the tile's sequence from here on
    const int tmax = pos0 + b0 + nb - 1, ntile = tmax / 64 + 1;
    if (split >= ntile) return;
    const float sqrt_hs = (float)sqrt((double)HS);
    const v16f_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    typedef float v4f_native __attribute__((ext_vector_type(4)));
    v4f_native kp[KPT];
#define SCM_KLOAD(TILE_) do { const int t0_ = 64 * (TILE_), rows_ = max(1, min(64, tmax + 1 - t0_)); \
        static_for<0, KPT, 1>([&](auto jc) { constexpr int j = decltype(jc)::value; const int i = t + NT * j, r = i / H4, c = i % H4; \
            kp[j] = *reinterpret_cast<const v4f_native*>(kc + (size_t)(min(t0_, tmax) + min(r, rows_ - 1)) * kv_dim + kvh * HS + 4 * c); }); } while (0)
    SCM_KLOAD(split);
    for (int i = t; i < ROWS * H4; i += NT) {                        // query rows (tokens past the chunk's end repeat its last token: never stored)
        const int row = i / H4, c = i % H4;
        const float4 x = *reinterpret_cast<const float4*>(Q + (size_t)(b0 + min(row & (SCM_TB - 1), nb - 1)) * q_stride + (size_t)hg.head_of(row >> 4) * HS + 4 * c);
        float* d = qs + row * QP + 4 * c;
        *reinterpret_cast<float2*>(d) = make_float2(x.x, x.y);
        *reinterpret_cast<float2*>(d + 2) = make_float2(x.z, x.w);
    }
    const float* qrow = qs + (16 * (2 * rp + rsel) + li) * QP + par;
    for (int tile = split; tile < ntile; tile += nsplit) {
        const int t0 = 64 * tile, t1 = min(tmax + 1, t0 + 64);
        static_for<0, KPT, 1>([&](auto jc) { constexpr int j = decltype(jc)::value; const int i = t + NT * j, r = i / H4, c = i % H4;
            *reinterpret_cast<v4f_native*>(kt + r * PITCH + 4 * c) = kp[j]; });
        __syncthreads();
        SCM_KLOAD(min(tile + nsplit, ntile - 1));                    // unconditional; the last trip re-reads a tile it does not use
        float mrow[2] = {-INFINITY, -INFINITY};
        if (t0 + 16 * tq <= tmax) {                                  // this wavefront's 16 timesteps hold at least one attended position
            const float* krow = kt + min(16 * tq + li, t1 - t0 - 1) * PITCH;
            v8f_native sc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // [0..3] row group 2 rp, [4..7] row group 2 rp + 1 (row li of each); timesteps 16 tq + 4 lq + r
            F3_SCORE_TILE(krow, (void)0);
#pragma unroll
            for (int rgp = 0; rgp < 2; ++rgp) {
                const int tb = li, head = hg.h0 + 2 * rp + rgp, b = b0 + tb;
                const int ts0 = t0 + 16 * tq + 4 * lq, lim = tb < nb && hg.real(2 * rp + rgp) ? pos0 + b : -1;       // attended: ts <= lim (a surplus head slot: nothing)
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[r] = att_mul != 0.f ? sc[4 * rgp + r] * att_mul : sc[4 * rgp + r] / sqrt_hs;
                    if (ts0 + r <= lim) mrow[rgp] = fmaxf(mrow[rgp], v[r]);
                }
                float* o = att + ((size_t)b * n_heads + head) * ctx + ts0;
                if (ts0 + 3 <= lim) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (ts0 + r <= lim) o[r] = v[r];
                }
            }
        }
        if (tmx) {                                                   // the quarter's maximum per row: fold the four 16-lane rows, one slot per (quarter, row)
#pragma unroll
            for (int rgp = 0; rgp < 2; ++rgp) {
                float m = mrow[rgp];
                m = fmaxf(m, __shfl_xor(m, 16, 64)); m = fmaxf(m, __shfl_xor(m, 32, 64));
                if (lq == 0) mxs[tq * ROWS + 16 * (2 * rp + rgp) + li] = m;
            }
        }
        __syncthreads();
        if (tmx && t < ROWS) {
            const int tb = t & (SCM_TB - 1), b = b0 + tb;
            if (tb < nb && hg.real(t >> 4) && t0 <= pos0 + b) {
                const float m = fmaxf(fmaxf(mxs[t], mxs[ROWS + t]), fmaxf(mxs[2 * ROWS + t], mxs[3 * ROWS + t]));
                tmx[((size_t)b * n_heads + hg.h0 + (t >> 4)) * tmx_tiles + tile] = m;
            }
        }
    }
#undef SCM_KLOAD
}

// LDS attributes of the prefill attention kernels (both plan kinds)
static int32_t pf_attention_attributes(gl3_ctx* ctx) {
#define GL3_ATTR150(K_) GL3_HIP(hipFuncSetAttribute((const void*)K_, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PF_ATTN_LDS_MAX))
    GL3_ATTR150(pf_attn_fused_kernel<128>); GL3_ATTR150(pf_attn_fused_kernel<64>); GL3_ATTR150(pf_attn_fused_kernel<32>);
    GL3_ATTR150(pf_attn_fused2_kernel<128>); GL3_ATTR150(pf_attn_fused2_kernel<64>); GL3_ATTR150(pf_attn_fused2_kernel<32>);
    GL3_ATTR150(pf_attn_fused3_kernel<128>); GL3_ATTR150(pf_attn_fused3_kernel<64>);
    // the run-table forms (mixed steps, gl3_forward_batch)
    GL3_ATTR150((pf_attn_fused2_kernel<128, true>)); GL3_ATTR150((pf_attn_fused2_kernel<64, true>)); GL3_ATTR150((pf_attn_fused2_kernel<32, true>));
    GL3_ATTR150((pf_attn_fused3_kernel<128, true>)); GL3_ATTR150((pf_attn_fused3_kernel<64, true>));
    GL3_ATTR150(pf_scores_mfma_kernel<128>); GL3_ATTR150(pf_scores_mfma_kernel<64>); GL3_ATTR150(pf_pv_mfma_kernel<128>); GL3_ATTR150(pf_pv_mfma_kernel<64>);
    GL3_ATTR150((pf_scores_pk_kernel<128, 4>)); GL3_ATTR150((pf_scores_pk_kernel<128, 2>)); GL3_ATTR150((pf_scores_pk_kernel<128, 1>));
    GL3_ATTR150((pf_scores_pk_kernel<64, 4>)); GL3_ATTR150((pf_scores_pk_kernel<64, 2>)); GL3_ATTR150((pf_scores_pk_kernel<64, 1>));
    GL3_ATTR150((pf_scores_pk_kernel<32, 4>)); GL3_ATTR150((pf_scores_pk_kernel<32, 2>)); GL3_ATTR150((pf_scores_pk_kernel<32, 1>));
    GL3_ATTR150((pf_scores_pk_kernel<96, 4>)); GL3_ATTR150((pf_scores_pk_kernel<96, 2>)); GL3_ATTR150((pf_scores_pk_kernel<96, 1>));
    // the run-table forms of the long-context kernels (the deep rows of a mixed step)
    GL3_ATTR150((pf_scores_mfma_kernel<128, true>)); GL3_ATTR150((pf_scores_mfma_kernel<64, true>)); GL3_ATTR150((pf_pv_mfma_kernel<128, true>)); GL3_ATTR150((pf_pv_mfma_kernel<64, true>));
    GL3_ATTR150((pf_scores_pk_kernel<128, 4, true>)); GL3_ATTR150((pf_scores_pk_kernel<128, 2, true>)); GL3_ATTR150((pf_scores_pk_kernel<128, 1, true>));
    GL3_ATTR150((pf_scores_pk_kernel<64, 4, true>)); GL3_ATTR150((pf_scores_pk_kernel<64, 2, true>)); GL3_ATTR150((pf_scores_pk_kernel<64, 1, true>));
    GL3_ATTR150((pf_scores_pk_kernel<32, 4, true>)); GL3_ATTR150((pf_scores_pk_kernel<32, 2, true>)); GL3_ATTR150((pf_scores_pk_kernel<32, 1, true>));
    GL3_ATTR150((pf_scores_pk_kernel<96, 4, true>)); GL3_ATTR150((pf_scores_pk_kernel<96, 2, true>)); GL3_ATTR150((pf_scores_pk_kernel<96, 1, true>));
#undef GL3_ATTR150
    return GL3_OK;
}
