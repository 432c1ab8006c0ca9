// gl3_kquant_gemm.h — the batched GEMMs on native K-quant storage (GL3_FLAG_KQUANT_NATIVE_BATCH): matrices whose Q4_K / Q5_K / Q6_K row
// segments stay at 19 / 23.25 / 28 bytes per block in HBM (gl3_kquant_kernels.h) under batched prefill, static-batched decode and mixed steps,
// bit-equal to the Q8T kernels on the converted plan.  Every Q8_0 block is rebuilt by kq_load / kq_rebuild, the int8 dot is exact, and
// the f32 steps are those of bdw_gemm_kernel: p = (float)isum * (wScale * aScale), acc += p, blocks ascending, then the epilogue.
//
// Steps of at most 64 tokens: kq_gemm_kernel.  bdw_gemm_kernel is one wavefront per (strip, 16-token tile); on native storage each
// token tile would repeat the rebuild — a few hundred VALU instructions per block, the cost that dominates — so here a workgroup of
// four wavefronts owns a strip (SwiGLU: the gate strip and the up strip) and rebuilds every block ONCE for all token tiles:
//   * K is cut into stages of KQG_STAGE = 4 tiles (512 elements), one tile per wavefront and matrix: lane l = (row l & 15, block l >> 4)
//     loads its slot (one coalesced load per field, non-temporal: nothing re-reads the strip), rebuilds it and writes the 32 int8 codes
//     and the widened scale into the stage's LDS slot.
//   * The codes lie in the A-operand order of v_mfma_i32_16x16x32_i8: per block the 8-byte k-chunk of lane (row r, k-group g) at
//     ((4 block + g) * 16 + r) * 8, chunk c(g) = k 0-7, 16-23, 8-15, 24-31 — the order XQ2 is pre-split for (bdq_offset), so the B side
//     is read exactly as bdw_gemm_kernel reads it.  A consumer's read of a block is 512 contiguous bytes of the wavefront, its scales one
//     broadcast float4 = the four rows a lane accumulates.
//   * Wavefront t < ceil(ntok / 16) owns token tile t: per block of the stage one MFMA and four (mul, mul, add), results in registers
//     across all of K.  A wavefront without a token tile only rebuilds (its activation loads go to a valid slot and are not used).
//   * Two LDS stage slots, one workgroup barrier per stage: slot s & 1 is written in iteration s after the barrier of iteration s - 1,
//     which every wavefront reaches only after it has consumed stage s - 2.  The weight loads of stage s + 1 and the activation loads of
//     stage s are issued before the rebuild of stage s, unconditionally; past the end of K the tile index is clamped (the duplicate tile
//     is rebuilt into a slot nobody consumes), so nothing is read behind a strip and no load sits under a condition inside the loop.
//   * The format of a strip is a wave-uniform value from the launch's KqRec: Q4_K | Q4_K | Q6_K or Q5_K | Q5_K | Q6_K segments of a fused qkv, a
//     SwiGLU pair of two formats, Q8T segments beside native ones (Q8_0 tensors of the same file; kq_load reads them, the "rebuild" is a move).
//   * Grid: one workgroup per strip.  bdw_grid's XCD rule co-locates the token tiles of a strip; here they are one workgroup.
//   * Epilogues: EPI_STORE (out_scale; the logits), EPI_RESID, EPI_SWIGLU writing f32 (the layer code quantises hb with its own launch).
//
// Steps of more than 64 tokens: kq_expand_q8t_kernel rebuilds a row slab of a native matrix into Q8T tiles in a scratch buffer — the
// inverse of kq_load's Q8T branch: the f16 scale header, the 16-byte halves at +128 and +1152, each field one coalesced store of the
// wavefront — and pf_gemm3_kernel / pf_gemm3t_kernel run on the slab as they are.  The rebuild is paid once per (row, block) and step.
#pragma once
#include "gl3_kquant_kernels.h"
#include "gl3_bd_gemm.h"

constexpr int KQG_STAGE = 4;                  // tiles per K stage = wavefronts per workgroup
constexpr int KQG_THREADS = 64 * KQG_STAGE;
constexpr int KQG_TILE_CODES = 64 * 32;       // int8 codes of one rebuilt tile

// The launch of one native GEMM of a step of at most 64 tokens: what launch_gemm launches for a matrix with native segments.
struct KqGemmPlan {
    int tslots, stage, threads, grid;          // TS (0: more than 64 tokens, not this kernel), tiles per stage, threads, workgroups = strips
    int ntt, ntiles, nstages, lds;             // token tiles (consuming wavefronts), K tiles, stages (the last may be ragged), static LDS bytes
};
inline KqGemmPlan kq_gemm_plan(int epi, int rows, int k, int ntok) {
    KqGemmPlan p{};
    p.tslots = bd_tslots(ntok);
    if (!p.tslots) return p;
    p.stage = KQG_STAGE; p.threads = KQG_THREADS; p.grid = (rows + 15) / 16;
    p.ntt = (ntok + 15) / 16;
    p.ntiles = (k / 32 + 3) / 4;
    p.nstages = (p.ntiles + KQG_STAGE - 1) / KQG_STAGE;
    p.lds = 2 * (epi == EPI_SWIGLU ? 2 : 1) * KQG_STAGE * (KQG_TILE_CODES + 64 * 4);
    return p;
}

// The K walk both kernels below run on one strip: this workgroup's four wavefronts rebuild the strip's tiles (matrix m: format fmt[m], first
// tile at wbase[m]) stage by stage and, if `consumer`, this wavefront accumulates its 16 tokens (lane r: token slot tokslot) in acc.
// TS: token slots of XQ2 / XS2 as a compile-time constant, or 0 for the run-time count ts (the grouped form).
template <int EPI, int TS>
__device__ __forceinline__ void kq_gemm_strip(const GemmArgs& a, const int (&fmt)[EPI == EPI_SWIGLU ? 2 : 1], const uint8_t* const (&wbase)[EPI == EPI_SWIGLU ? 2 : 1],
                                              bool consumer, uint32_t tokslot, int ts_rt, float (&acc)[EPI == EPI_SWIGLU ? 2 : 1][4]) {
    constexpr int NM = (EPI == EPI_SWIGLU) ? 2 : 1;
    __shared__ __attribute__((aligned(16))) uint8_t codes[2][NM][KQG_STAGE][KQG_TILE_CODES];
    __shared__ __attribute__((aligned(16))) float wsc[2][NM][KQG_STAGE][64];       // [block][row] weight scales of a tile
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ng = a.ng, ts = TS ? TS : ts_rt;
    const uint8_t* xq = a.XQ + tokslot * 64 + 16 * g;
    const float* xs = a.XS + tokslot * 4;
    KqRaw raw[NM];
    auto wload = [&](int s) __attribute__((always_inline)) {                      // this wavefront's tile of stage s, clamped into the strip
        const int tile = min(KQG_STAGE * s + wave, ng - 1);
#pragma unroll
        for (int m = 0; m < NM; ++m) raw[m] = kq_load(fmt[m], wbase[m] + (size_t)tile * kq_tile_bytes(fmt[m]), lane);
    };
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[m][i] = 0.f;
    const int nstages = (ng + KQG_STAGE - 1) / KQG_STAGE;
    wload(0);
    for (int s = 0; s < nstages; ++s) {
        const int slot = s & 1;
        KqRaw cur[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) cur[m] = raw[m];
        wload(s + 1);                                                               // clamped: the last iteration reloads the strip's last tile
        // the activations of stage s (L2): both block pairs and the four block scales of every tile, for this lane's token and k-group
        v2l_t B[KQG_STAGE][2]; float4 X[KQG_STAGE];
#pragma unroll
        for (int j = 0; j < KQG_STAGE; ++j) {
            const int tile = min(KQG_STAGE * s + j, ng - 1);
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) B[j][jj] = *reinterpret_cast<const v2l_t*>(xq + ((size_t)tile * 2 + jj) * ((size_t)ts * 64));
            X[j] = *reinterpret_cast<const float4*>(xs + (size_t)tile * ((size_t)ts * 4));
        }
        // rebuild: lane (row r, block g) of tile `wave` -> its four k-chunks in operand order, and its scale
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const KqBlock q = kq_rebuild(fmt[m], cur[m]);
            uint8_t* c = codes[slot][m][wave];
            *reinterpret_cast<kq2i*>(c + ((4 * g + 0) * 16 + r) * 8) = (kq2i){q.lo.x, q.lo.y};      // k 0-7
            *reinterpret_cast<kq2i*>(c + ((4 * g + 1) * 16 + r) * 8) = (kq2i){q.hi.x, q.hi.y};      // k 16-23
            *reinterpret_cast<kq2i*>(c + ((4 * g + 2) * 16 + r) * 8) = (kq2i){q.lo.z, q.lo.w};      // k 8-15
            *reinterpret_cast<kq2i*>(c + ((4 * g + 3) * 16 + r) * 8) = (kq2i){q.hi.z, q.hi.w};      // k 24-31
            wsc[slot][m][wave][lane] = q.ws;                                        // lane = 16 block + row
        }
        wg_barrier();
        if (consumer) {
#pragma unroll
            for (int j = 0; j < KQG_STAGE; ++j) {
                if (KQG_STAGE * s + j >= ng) break;                                 // ragged last stage (wave-uniform)
                const float xv[4] = {X[j].x, X[j].y, X[j].z, X[j].w};
#pragma unroll
                for (int bi = 0; bi < 4; ++bi) {
                    const long bop = B[j][bi >> 1][bi & 1];
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const long aop = *reinterpret_cast<const long*>(codes[slot][m][j] + ((4 * bi + g) * 16 + r) * 8);
                        const v4i_t c = __builtin_amdgcn_mfma_i32_16x16x32_i8(aop, bop, (v4i_t){0, 0, 0, 0}, 0, 0, 0);
                        const float4 w4 = *reinterpret_cast<const float4*>(&wsc[slot][m][j][16 * bi + 4 * g]);
                        acc[m][0] = acc[m][0] + (float)c[0] * (w4.x * xv[bi]);      // result += isum * (wScale * aScale)
                        acc[m][1] = acc[m][1] + (float)c[1] * (w4.y * xv[bi]);
                        acc[m][2] = acc[m][2] + (float)c[2] * (w4.z * xv[bi]);
                        acc[m][3] = acc[m][3] + (float)c[3] * (w4.w * xv[bi]);
                    }
                }
            }
        }
    }
}
// o[i] = the epilogue of rows rbase .. rbase + 3 of one token (C layout: a lane holds weight rows 4g .. 4g + 3 of its token)
template <int EPI>
__device__ __forceinline__ void kq_gemm_store(const GemmArgs& a, float* o, int rbase, const float (&acc)[EPI == EPI_SWIGLU ? 2 : 1][4]) {
    constexpr int NM = (EPI == EPI_SWIGLU) ? 2 : 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (rbase + i >= a.rows) continue;
        const float v0 = acc[0][i];
        if (EPI == EPI_SWIGLU) {
            const float gt = v0 / (float)(1.0 + exp(-(double)v0));
            o[i] = gt * acc[NM - 1][i];
        } else if (EPI == EPI_STORE) o[i] = v0 * a.out_scale;
        else o[i] = o[i] + v0 * a.out_scale;
    }
}

template <int EPI, int TS>
__global__ GL3_NO_PK_F32 __launch_bounds__(KQG_THREADS) void kq_gemm_kernel(const GemmArgs a, const KqRec kr) {
    constexpr int NM = (EPI == EPI_SWIGLU) ? 2 : 1;
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strip = blockIdx.x, ng = a.ng;
    const bool consumer = 16 * wave < a.ntok;                                      // wave-uniform
    const uint32_t tokslot = 16 * min(wave, TS / 16 - 1) + r;                      // a wavefront without a token tile reads a valid slot
    // the strip's segment and format per matrix (scalar)
    const int first1 = __builtin_amdgcn_readfirstlane(kr.seg[1].first_strip), first2 = __builtin_amdgcn_readfirstlane(kr.seg[2].first_strip);
    const int si = strip >= first2 ? 2 : strip >= first1 ? 1 : 0;
    const uint8_t* sbase = si == 2 ? kr.seg[2].base : si == 1 ? kr.seg[1].base : kr.seg[0].base;
    const int sfirst = si == 2 ? first2 : si == 1 ? first1 : 0;
    int fmt[NM]; const uint8_t* wbase[NM];
    fmt[0] = __builtin_amdgcn_readfirstlane(si == 2 ? kr.seg[2].fmt : si == 1 ? kr.seg[1].fmt : kr.seg[0].fmt);
    wbase[0] = kq_uniform(sbase) + (size_t)(strip - sfirst) * ng * kq_tile_bytes(fmt[0]);
    if (NM == 2) {
        fmt[NM - 1] = __builtin_amdgcn_readfirstlane(kr.seg2.fmt);
        wbase[NM - 1] = kq_uniform(kr.seg2.base) + (size_t)strip * ng * kq_tile_bytes(fmt[NM - 1]);
    }
    float acc[NM][4];
    kq_gemm_strip<EPI, TS>(a, fmt, wbase, consumer, tokslot, 0, acc);
    // epilogue.  C layout: token = 16 wave + (lane & 15), weight rows 4g .. 4g + 3 of the strip
    const int b = 16 * wave + r;
    if (!consumer || b >= a.ntok) return;
    const int rbase = strip * 16 + 4 * g;
    kq_gemm_store<EPI>(a, a.out + (size_t)b * a.out_stride + rbase, rbase, acc);
}

// ---------------------------------------------------------------------------------------------------
// The routed experts of a Qwen2-MoE step on native stacked tensors (GL3_FLAG_KQUANT_NATIVE_MOE): kq_gemm_kernel over moe_group_kernel's tile
// table.  bdw_gemm_kernel<.., GRP> is one wavefront per (table entry, strip) and would rebuild a strip once per entry; here a workgroup
// owns (expert, strip, up to four consecutive entries of that expert = 64 sorted slots), rebuilds every stage once, and wavefront t
// consumes entry t: token slots gathered through gtok, result rows scattered through gdst, as the GRP form does, the products and
// their order those of bdw_gemm_kernel.  An expert with more than four entries takes further workgroups, each rebuilding again.
//   * Grid: workgroup id = entry * gspe + strip over the bound moe_group_max_entries(), as the GRP form (the step stays one graph).
//     Entry u leads a workgroup when its index within its expert is a multiple of four; that index is the number of entries in front
//     of u with u's expert — the table lists an expert's entries consecutively — counted 64 per ballot.  Surplus workgroups and the
//     other entries exit at once.
//   * The token-slot count of XQ2 / XS2 is the run-time a.tslots (any chunk length), so one kernel serves every step size: nothing is
//     expanded into the Q8T scratch.  The stacked tensor is one segment (s0; SwiGLU: s1 = up), expert e at strip e * gspe of it; a
//     Q8T stack beside a native one is read through kq_load like any Q8T segment.
template <int EPI>
__global__ GL3_NO_PK_F32 __launch_bounds__(KQG_THREADS) void kq_gemm_grp_kernel(const GemmArgs a, const KqSeg s0, const KqSeg s1) {
    constexpr int NM = (EPI == EPI_SWIGLU) ? 2 : 1;
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int u = blockIdx.x / a.gspe, strip = blockIdx.x % a.gspe, nent = a.gtab[0];
    if (u >= nent) return;                                                          // the grid is sized for the bound on the table
    const int e = a.gtab[4 + 4 * u];
    int ahead = 0;                                                                  // entries of expert e in front of entry u
    for (int u0 = u - 1;; u0 -= 64) {
        const int v = u0 - lane;
        const unsigned long long same = __builtin_amdgcn_ballot_w64(v >= 0 && a.gtab[4 + 4 * v] == e);
        const int run = same == ~0ull ? 64 : __builtin_ctzll(~same);
        ahead += run;
        if (run < 64) break;
    }
    if (ahead & 3) return;
    const int mine = u + wave;                                                      // wavefront t consumes entry u + t, if it is expert e's
    const bool consumer = mine < nent && a.gtab[4 + 4 * mine] == e;                 // wave-uniform
    const int4 en = *reinterpret_cast<const int4*>(a.gtab + 4 + 4 * (consumer ? mine : u));      // a wavefront without an entry reads valid slots
    const int gcnt = en.z, gslot = en.y + min(r, gcnt - 1);                         // lanes past the ragged end: the last valid slot
    const uint32_t tokslot = a.gtok ? a.gtok[gslot] : gslot;
    int fmt[NM]; const uint8_t* wbase[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        fmt[m] = __builtin_amdgcn_readfirstlane(m ? s1.fmt : s0.fmt);
        wbase[m] = kq_uniform(m ? s1.base : s0.base) + ((size_t)e * a.gspe + strip) * a.ng * kq_tile_bytes(fmt[m]);
    }
    float acc[NM][4];
    kq_gemm_strip<EPI, 0>(a, fmt, wbase, consumer, tokslot, a.tslots, acc);
    if (!consumer || r >= gcnt) return;
    const int rbase = strip * 16 + 4 * g;                                           // row of the expert's own output
    kq_gemm_store<EPI>(a, a.out + (size_t)(a.gdst ? a.gdst[gslot] : gslot) * a.out_stride + rbase, rbase, acc);
}

// ---------------------------------------------------------------------------------------------------
// Embedding rows of a native token_embd for the tokens of a batched step: x[i] = ((float)q8[i] * d8) * emb_scale of the rebuilt blocks —
// pf_embed_kernel's arithmetic, embed_kq_kernel's source.  One workgroup per token, one thread per 32-block of the row; X in the
// rank-chunked layout (chunk width cc).
static __global__ GL3_NO_PK_F32 __launch_bounds__(256) void pf_embed_kq_kernel(const uint8_t* __restrict__ emb, int fmt, int ng, int dim,
                                                                         const int32_t* __restrict__ tokens, float* __restrict__ X, int cc, float emb_scale) {
    const int token = tokens[blockIdx.x];
    const uint8_t* strip = emb + (size_t)(token >> 4) * ng * kq_tile_bytes(fmt);
    const int bt = blockIdx.x, nt = gridDim.x;
    for (int b = threadIdx.x; b < (dim >> 5); b += 256) {
        const KqBlock q = kq_rebuild(fmt, kq_load(fmt, strip + (size_t)(b >> 2) * kq_tile_bytes(fmt), (token & 15) + 16 * (b & 3)));
        const int w[8] = {q.lo.x, q.lo.y, q.lo.z, q.lo.w, q.hi.x, q.hi.y, q.hi.z, q.hi.w};
#pragma unroll
        for (int e = 0; e < 32; ++e) X[chunked(bt, 32 * b + e, cc, nt)] = ((float)(int8_t)(w[e >> 2] >> (8 * (e & 3))) * q.ws) * emb_scale;
    }
}

// ---------------------------------------------------------------------------------------------------
// ntiles tiles of one row segment (whole strips, format fmt) -> Q8T tiles at dst.  One wavefront per tile, lane l = its (row, block) slot.
static __global__ GL3_NO_PK_F32 __launch_bounds__(256) void kq_expand_q8t_kernel(const uint8_t* __restrict__ src, int fmt, long ntiles, uint8_t* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const KqBlock q = kq_rebuild(fmt, kq_load(fmt, src + (size_t)tile * kq_tile_bytes(fmt), lane));
    uint8_t* t = dst + (size_t)tile * TILE_BYTES;
    *reinterpret_cast<uint16_t*>(t + 2 * lane) = __builtin_bit_cast(uint16_t, (_Float16)q.ws);
    *reinterpret_cast<kq4i*>(t + 128 + 16 * lane) = q.lo;
    *reinterpret_cast<kq4i*>(t + 1152 + 16 * lane) = q.hi;
}
