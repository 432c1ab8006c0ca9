// gl3_prefill.hip — batched prefill (gl3_forward_prefill with max_batch > 1) and static-batched decode
// (gl3_forward_decode_batch) and the mixed step (gl3_forward_batch); tensor-parallel ranks keep gathered activations rank-chunked
// (see `chunked`, gl3_chunked.h).
//
// Replaces the reference's batched-prefill task graphs
//   J/tornadovm/layers/type/q8_0/prefill/LlamaQ8_0LayersBatchPrefillMMA.java:84-219 (tensor-core path, CUDA only) and
//   ...LlamaQ8_0LayersBatchPrefill.java (scalar path), kernels in J/tornadovm/kernels/TransformerBatchPrefillKernels.java
// but computes what the CPU path computes, bit for bit: InferenceCoreBatchPrefillDecode.batchForwardJavaPrefill
// (J/inference/InferenceCoreBatchPrefillDecode.java:62-168) = per token exactly forwardJava without the logits.
// The reference's MMA path is W8A16 (f16 activations); the CPU oracle is W8A8 with per-32-block int8 activations
// (Q8_0FloatTensor.java:90-123), and that is what the GEMM below does on CDNA4's int8 matrix cores:
//   one v_mfma_i32_32x32x32_i8 = the int32 dot of one Q8_0 block for a 32-row x 32-token tile (exact), then
//   acc = acc + float(isum) * (wScale * aScale) on the VALU, blocks ascending — the reference's f32 order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gl3_ctx.h"
#include "gl3_batch_plan.h"
#include "gl3_chunked.h"      // chunked(): the rank-chunked layout of every gathered activation
#include <type_traits>
#include "gl3_decode_kernels.h"

#include "gl3_prefill_vl.h"

using namespace gl3;
#include "gl3_bd_gemm.h"      // GemmArgs, bdw_gemm_kernel (expects the gl3 names in scope)
#include "gl3_moe_kernels.h"  // Qwen2-MoE: batched router, grouping, combine
#include "gl3_prefill_gemm3.h"      // g3_scale_operands (the kernels of that header are instantiated in gl3_prefill_gemm3.hip only)
// gl3_prefill_gemm3.hip (own translation unit, -fno-slp-vectorize): the > 64-token GEMM, every class (gl3_prefill_gemm3.h / gl3_prefill_gemm3t.h)
void gl3_gemm3_launch(int epi, const GemmArgs& a, int rows, int ntok, hipStream_t s);
bool gl3_gemm3_swiglu_quantises(int rows, int ntok);
hipError_t gl3_gemm3_allow_lds();

struct gl3_prefill_state {
    int max_batch = 0;
    int32_t* tokens = nullptr;          // [M]
    float* X = nullptr;                 // [M][dim] residual stream (rank-chunked [tp][n][dim/tp] under tensor parallelism)
    // The next GEMM's activation operand, in one of two layouts chosen by the step's token count n (pf_chunk_major):
    //   n <= 64 (bdw_gemm_kernel):  XQ / XS in the wave-owned layout of gl3_bd_gemm.h (bdq_offset / bds_offset, 32 or 64 token slots)
    //   n >  64 (pf_gemm3*_kernel): XQ chunk-major + the scales in XP; XS is not used
    uint8_t* XQ = nullptr;              // int8 activations; chunk-major: [maxk/16 + 8][xp_tok][16 B]
    float* XS = nullptr;                // activation scales, one f32 per 32-element block (small-batch layout only)
    uint8_t* XP = nullptr;              // chunk-major: [maxk/32 + 4][2 lane halves][xp_tok][16 B] the activation scales as bf16 MFMA operands
    int xp_tok = 0;                     //   token slots per block: max_batch rounded up to the GEMM's 128-token tile
    uint8_t* XQh = nullptr;             // second operand set of the > 64-token path: hb quantised by the gate + up GEMM's own epilogue (pf_gemm3t_kernel<.., QOUT>)
    uint8_t* XPh = nullptr;             //   while other workgroups still read XQ / XP
    uint8_t* XQb = nullptr;             // second small-batch operand buffer: hb quantised by the gate/up kernel's own epilogue
    float* XSb = nullptr;               //   (its input still being read by other workgroups)
    float* QKV = nullptr;               // [M][q_dim + 2 kv_dim]
    float* AO = nullptr;                // [M][q_dim] attention output (rank-chunked)
    float* HB = nullptr;                // [M][hidden] (rank-chunked)
    float* ATT = nullptr;               // [M][n_heads][ctx] scores
    float* TMX = nullptr;               // [M][n_heads][tmx_tiles] per-64-timestep-tile maxima of the score rows (the scores kernels -> pf_softmax_rows_kernel)
    float* SUMS = nullptr;              // [M][n_heads] softmax denominators (pf_softmax_rows_kernel -> pf_pv_mfma_kernel / pf_pv_ring_kernel)
    int tmx_tiles = 0;
    int32_t* seqpos = nullptr;          // [2][M]: sequence id, position of every token of the step
    // mixed steps (gl3_forward_batch): the attention tile table and the output rows of the step, staged with the tokens
    int4* tiles = nullptr;              // [M] BatchSpan records, deepest tile first (gl3_batch_plan.h); PfStep::ntab of them belong to the step
    int4* deep = nullptr;               // [M] the deep records of the step (batch_plan_split), deepest first; PfStep::ndeep of them
    int32_t* deep_rows = nullptr;       // [M] the step rows of the deep records, ascending; PfStep::deep_rows of them
    int tab_max_pos = 0;                // last position a tile may have in the one-launch table form (pf_tab_max_pos; INT_MAX: steps are not split)
    int32_t attn_rows[4] = {0, 0, 0, 0};      // rows of the last batched step by attention form (gl3_get_attn_rows), from the last layer's pf_attention
    bool attn_rows_set = false;
    int32_t* out_rows = nullptr;        // [M] rows whose logits are wanted
    float* XG = nullptr;                // [M][dim] those rows of X, compact (allocated by the first mixed step)
    float* LOGITS = nullptr;            // [rows][vocab], grown on demand (batched decode)
    int logits_rows = 0;
    std::vector<hipGraphExec_t> step_graphs;   // static-batched decode: one captured step per batch size (positions < AF_MAXN)
    bool in_arena = false;              // X / AO / HB / LOGITS are slices of the tensor-parallel arena (not freed here)
    int32_t* amax = nullptr;            // [M]
    float* amx_v = nullptr;             // [M][AMX_SPLIT] partial maxima of the greedy scan
    int* amx_i = nullptr;
    int maxk = 0;
    // F16 / Q4_0 / Q8_0-with-f32-activation plans (gl3_prefill_vl.h): the GEMMs read f32 activations
    bool vl = false;
    float* XN = nullptr;                // [M][dim] RMS-normalised activations
    float* HB2 = nullptr;               // [M][hidden] up projection (hb = silu(HB) * HB2)
    // Qwen2-MoE (pf_moe_ffn): the routing of every token of the step, its grouping by expert, and the routed experts' operands
    struct {
        float* logits = nullptr;        // [M][n_experts] router logits (scratch between the router's workgroups)
        float* w = nullptr;             // [M][topk + 1] routing weights, last = the shared expert's sigmoid gate
        int* sel = nullptr;             // [M][topk] expert ids
        int* ticket = nullptr;          // [M] arrival counters of the router (0 between launches)
        int* slot_tok = nullptr;        // [M topk] token of every sorted slot      } moe_group_kernel
        int* slot_dst = nullptr;        // [M topk] row of y of every sorted slot   }
        int* tab = nullptr;             // tile table: 4 ints header + 4 per entry  }
        float* HB = nullptr;            // [M topk][moe_hidden] routed hb, sorted-slot order
        float* Y = nullptr;             // [M][topk + 1][dim] down-projected outputs, last = the shared expert
        uint8_t* XQx = nullptr;         // xb of a > 64-token step in the XQ2 / XS2 layout with ts_x token slots (the chunk-major
        float* XSx = nullptr;           //   operand next to it serves the shared expert)
        uint8_t* XQh = nullptr;         // routed hb quantised, XQ2 / XS2 layout with ts_h token slots (slot = sorted slot)
        float* XSh = nullptr;
        int ts_x = 0, ts_h = 0;
    } moe;
};


// ---------------------------------------------------------------------------------------------------
// token_embedding_table.copyTo per token (batchForwardJavaPrefill :96), written in the rank-chunked layout (chunked(), gl3_chunked.h)
__global__ __launch_bounds__(256) void pf_embed_kernel(const uint8_t* __restrict__ emb, int ng, int dim,
                                                        const int32_t* __restrict__ tokens, float* __restrict__ X, int cc, float emb_scale) {
    const int token = tokens[blockIdx.x];
    const uint8_t* strip = emb + (size_t)(token >> 4) * ng * TILE_BYTES;
    const int i16 = token & 15;
    const int bt = blockIdx.x, nt = gridDim.x;
    for (int i = threadIdx.x; i < dim; i += 256) {
        const int b = i >> 5, j = i & 31;
        const uint8_t* p = strip + (size_t)(b >> 2) * TILE_BYTES;
        const int l = i16 + 16 * (b & 3);
        const float d = h2f(*reinterpret_cast<const uint16_t*>(p + 2 * l));
        const int8_t q = (int8_t)p[(j < 16 ? 128 : 1152) + 16 * l + (j & 15)];
        X[chunked(bt, i, cc, nt)] = ((float)q * d) * emb_scale;
    }
}

// ---------------------------------------------------------------------------------------------------
// Per token: (RMSNorm with the exact in-order sum of squares) + Q8_0 activation quantisation.
// One workgroup of 256 threads per token (PQ_NORM) or per (token, 1024-element chunk) (the other modes: the blocks are
// independent, and one workgroup per token left 32 tokens on 32 CUs).
//   PQ_PLAIN:  quantise an f32 row;  PQ_NORM: RMSNorm, then quantise
//   PQ_NORM_F32: RMSNorm only, f32 out (XS = [ntok][k] floats; the f32-activation weight types, gl3_prefill_vl.h)
enum { PQ_PLAIN = 0, PQ_NORM = 1, PQ_NORM_F32 = 2, PQ_PLAIN_F32 = 3 };     // PQ_PLAIN_F32: rank-chunked f32 row -> plain f32 row (XS)
template <int MODE>
__global__ __launch_bounds__(256) void pf_norm_quant_kernel(const float* __restrict__ in, int k, int in_stride,
                                                             const float* __restrict__ norm_w, float eps,
                                                             uint8_t* __restrict__ XQ, float* __restrict__ XS, int maxk, int tslots,
                                                             uint2* __restrict__ XP = nullptr, int xp_tok = 0) {
    constexpr bool NORM = MODE == PQ_NORM || MODE == PQ_NORM_F32;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* xf = reinterpret_cast<float*>(smem);                 // [k + 32]
    uint8_t* scratch = smem + (size_t)(k + 32) * 4;             // ss_scratch_bytes(k)
    float* red = reinterpret_cast<float*>(scratch + ss_scratch_bytes(k));
    const int t = threadIdx.x, b = blockIdx.x;
    const int cc = in_stride, nt = gridDim.x;                    // in_stride = chunk columns (k / tp); cc % 4 == 0
    auto xquad = [&](int qd) { return *reinterpret_cast<const float4*>(in + chunked(b, 4 * qd, cc, nt)); };
    const int nquads = k >> 2;
    float scale = 1.0f;
    if (NORM) {
        for (int qd = t; qd < nquads; qd += 256)
            *reinterpret_cast<float4*>(xf + 4 * qd) = xquad(qd);
        if (t < 32) xf[k + t] = 0.f;
        __syncthreads();
        float ss;
        if (k >= 1024 && k <= 5120) {
            BlockBarrier bb;
            ss = exact_sumsq_lds(xf, k, scratch, t, bb);
        } else {
            if (t < 64) { const float s1 = seq_sum_lds<true>(xf, k); if (t == 0) red[0] = s1; }
            __syncthreads();
            ss = red[0];
        }
        ss /= (float)k;
        ss += eps;
        scale = (float)(1.0 / sqrt((double)ss));
    }
    for (int qd = t + 256 * blockIdx.y; qd < nquads; qd += 256 * gridDim.y) {
        float4 v;
        if (NORM) {
            v = *reinterpret_cast<const float4*>(xf + 4 * qd);
            const float4 w = *reinterpret_cast<const float4*>(norm_w + 4 * qd);
            v.x = w.x * (scale * v.x); v.y = w.y * (scale * v.y); v.z = w.z * (scale * v.z); v.w = w.w * (scale * v.w);
        } else {
            v = xquad(qd);
        }
        if (MODE == PQ_NORM_F32 || MODE == PQ_PLAIN_F32) { *reinterpret_cast<float4*>(XS + (size_t)b * k + 4 * qd) = v; continue; }
        if (tslots == 0) {                                 // chunk-major (pf_gemm3_kernel): int8 operand XQ[k / 16][xp_tok token slots][16 B], scales in XP
            float qs;
            const uint32_t packed = quantize_quad_pack(v, qs);
            *reinterpret_cast<uint32_t*>(XQ + ((size_t)(qd >> 2) * xp_tok + b) * 16 + 4 * (qd & 3)) = packed;
            if ((qd & 7) == 0) {
                const G3ScaleOperands so = g3_scale_operands(qs);      // the scale (an f16 value) as the bf16 operands the s / -B s MFMAs read
                const int blk = qd >> 3;
                uint4* xp = reinterpret_cast<uint4*>(XP);      // XP[block][half][xp_tok][16 B]
                xp[((size_t)blk * 2 + 0) * xp_tok + b] = so.half0;
                xp[((size_t)blk * 2 + 1) * xp_tok + b] = so.half1;
                // ragged K: the padded blocks of the last tile group carry zero weights; give them zero activation operands too
                if (blk == (k >> 5) - 1)
                    for (int pb = blk + 1; pb < ((blk + 4) & ~3); ++pb) {
                        xp[((size_t)pb * 2 + 0) * xp_tok + b] = make_uint4(0u, 0u, 0u, 0u);
                        xp[((size_t)pb * 2 + 1) * xp_tok + b] = make_uint4(0u, 0u, 0u, 0u);
                    }
            }
        } else {                                           // the wave-owned small-batch GEMM's operand layout (gl3_bd_gemm.h)
            float qs;
            const uint32_t packed = quantize_quad_pack(v, qs);
            *reinterpret_cast<uint32_t*>(XQ + bdq_offset(qd, b, tslots)) = packed;
            if ((qd & 7) == 0) XS[bds_offset(qd >> 3, b, tslots)] = qs;
        }
    }
}

#include "gl3_prefill_attn.h"

// Greedy id per sequence: first index of the maximum of each logits row (FloatTensor.argmax :138-151).
// logits: rank-chunked [tp][rows][n / tp] (cc = n / tp, a multiple of 4; tp = 1: plain rows).
// Two launches: (AMX_SPLIT segments x rows) workgroups scan their segment with float4 loads -> one (value, index) pair each; one
// wavefront per row folds the pairs.  (Round 2: one 1024-thread workgroup per row with scalar strided loads, 75 us per step for a
// 19 MB scan at B = 32 — 30x its HBM time.)
constexpr int AMX_SPLIT = 32;
__device__ __forceinline__ void amx_fold(float& best, int& idx, float ob, int oi) {
    if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
}
__global__ __launch_bounds__(256) void pf_argmax_part_kernel(const float* __restrict__ logits, int n, int cc, float* __restrict__ pv, int* __restrict__ pi) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int t = threadIdx.x, seg = blockIdx.x, row = blockIdx.y, nrows = gridDim.y;
    const int nq = n >> 2, per = (nq + AMX_SPLIT - 1) / AMX_SPLIT;
    const int q0 = seg * per, q1 = min(nq, q0 + per);
    float best = -INFINITY;
    int idx = 0x7FFFFFFF;
    for (int q = q0 + t; q < q1; q += 256) {
        const int i = 4 * q;
        const float4 f = *reinterpret_cast<const float4*>(logits + chunked(row, i, cc, nrows));
        if (f.x > best) { best = f.x; idx = i; }            // ascending i inside a thread: strict > keeps the first maximum
        if (f.y > best) { best = f.y; idx = i + 1; }
        if (f.z > best) { best = f.z; idx = i + 2; }
        if (f.w > best) { best = f.w; idx = i + 3; }
    }
    if (seg == AMX_SPLIT - 1)                               // n is a multiple of 16 in every supported shape; kept for safety
        for (int i = 4 * nq + t; i < n; i += 256) { const float f = logits[chunked(row, i, cc, nrows)]; if (f > best) { best = f; idx = i; } }
    for (int m = 32; m >= 1; m >>= 1) amx_fold(best, idx, __shfl_xor(best, m, 64), __shfl_xor(idx, m, 64));
    if ((t & 63) == 0) { bv[t >> 6] = best; bi[t >> 6] = idx; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; ++w) amx_fold(best, idx, bv[w], bi[w]);
        pv[row * AMX_SPLIT + seg] = best; pi[row * AMX_SPLIT + seg] = idx;
    }
}
__global__ __launch_bounds__(64) void pf_argmax_fold_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int32_t* __restrict__ out) {
    const int row = blockIdx.x, t = threadIdx.x;
    float best = t < AMX_SPLIT ? pv[row * AMX_SPLIT + t] : -INFINITY;
    int idx = t < AMX_SPLIT ? pi[row * AMX_SPLIT + t] : 0x7FFFFFFF;
    for (int m = 32; m >= 1; m >>= 1) amx_fold(best, idx, __shfl_xor(best, m, 64), __shfl_xor(idx, m, 64));
    if (t == 0) out[row] = idx == 0x7FFFFFFF ? 0 : idx;
}

// ------------------------------------------------------------------------------------------------ host side
// dynamic LDS of pf_norm_quant_kernel<PQ_NORM | PQ_NORM_F32> for rows of k elements: the row, the exact sum of squares' scratch, the result.
// Above 64 KB (k >= 9344) it needs the attribute gl3_prefill_alloc sets; gl3_create refuses a dim whose request exceeds that.
static size_t nq_smem(int k) { return (size_t)(k + 32) * 4 + ss_scratch_bytes(k) + 64; }
size_t gl3_prefill_norm_smem(int k) { return nq_smem(k); }
static int pf_tab_max_pos(const gl3_ctx* ctx);      // next to pf_attention, whose conditions it shares
int32_t gl3_prefill_alloc(gl3_ctx* ctx) {
    const gl3_model_desc& d = ctx->d;
    gl3_prefill_state* p = new gl3_prefill_state();
    ctx->pf = p;
    p->max_batch = d.max_batch;
    const size_t M = d.max_batch;
    p->vl = ctx->emb.vl;
    // every weight class: tokens, the f32 activations (the gathered ones in the arena the peers map under tensor parallelism), attention, greedy scan
    GL3_HIP(hipMalloc((void**)&p->tokens, M * sizeof(int32_t)));
    if (ctx->arena.base && ctx->arena.off[GB_PF_X]) {
        uint8_t* b = ctx->arena.base;
        p->X = (float*)(b + ctx->arena.off[GB_PF_X]); p->AO = (float*)(b + ctx->arena.off[GB_PF_AO]); p->HB = (float*)(b + ctx->arena.off[GB_PF_HB]);
        p->LOGITS = (float*)(b + ctx->arena.off[GB_PF_LOGITS]); p->logits_rows = ctx->arena.pf_logits_rows;
        p->in_arena = true;
    } else {
        GL3_HIP(hipMalloc((void**)&p->X, M * d.dim * 4));
        GL3_HIP(hipMalloc((void**)&p->AO, M * ctx->q_dim * 4));
        GL3_HIP(hipMalloc((void**)&p->HB, M * d.hidden * 4));
    }
    GL3_HIP(hipMalloc((void**)&p->QKV, M * (ctx->q_dim + 2 * ctx->kv_dim) * 4));
    GL3_HIP(hipMalloc((void**)&p->ATT, M * d.n_heads * (size_t)d.ctx * 4));
    p->tmx_tiles = (d.ctx + 63) / 64;
    GL3_HIP(hipMalloc((void**)&p->TMX, M * d.n_heads * (size_t)p->tmx_tiles * 4));
    GL3_HIP(hipMalloc((void**)&p->SUMS, M * d.n_heads * 4));
    GL3_HIP(hipMalloc((void**)&p->seqpos, 2 * M * sizeof(int32_t)));
    GL3_HIP(hipMalloc((void**)&p->tiles, M * sizeof(int4)));
    GL3_HIP(hipMalloc((void**)&p->deep, M * sizeof(int4)));
    GL3_HIP(hipMalloc((void**)&p->deep_rows, M * sizeof(int32_t)));
    GL3_HIP(hipMalloc((void**)&p->out_rows, M * sizeof(int32_t)));
    GL3_HIP(hipMalloc((void**)&p->amax, M * sizeof(int32_t)));
    GL3_HIP(hipMalloc((void**)&p->amx_v, M * AMX_SPLIT * sizeof(float)));
    GL3_HIP(hipMalloc((void**)&p->amx_i, M * AMX_SPLIT * sizeof(int)));
    GL3_HIP(hipFuncSetAttribute((const void*)pf_attn_scores_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    GL3_HIP(hipFuncSetAttribute((const void*)pf_attn_softmax_pv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    { const int32_t ar = pf_attention_attributes(ctx); if (ar != GL3_OK) return ar; }
    GL3_HIP(hipFuncSetAttribute((const void*)pf_norm_quant_kernel<PQ_NORM>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    GL3_HIP(hipFuncSetAttribute((const void*)pf_norm_quant_kernel<PQ_NORM_F32>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    p->tab_max_pos = pf_tab_max_pos(ctx);
    if (p->vl) {       // f32-activation weight types: the GEMMs read f32 rows, no int8 operands
        // XN: normalised / un-chunked f32 operand of the next GEMM (K up to max(dim, q_dim, hidden)); HB2: this rank's up projection
        const size_t kmax = (size_t)(d.hidden > ctx->q_dim ? (d.hidden > d.dim ? d.hidden : d.dim) : (ctx->q_dim > d.dim ? ctx->q_dim : d.dim));
        GL3_HIP(hipMalloc((void**)&p->XN, M * kmax * 4));
        GL3_HIP(hipMalloc((void**)&p->HB2, M * ctx->hidden_l * 4));
        if (getenv("GL3_DEBUG_ALLOC"))
            fprintf(stderr, "[gl3 alloc vl] M %zu tokens %p X %p XN %p AO %p HB %p HB2 %p QKV %p ATT %p seqpos %p amax %p (dim %d hidden %d qdim %d ctx %d)\n", M, (void*)p->tokens,
                    (void*)p->X, (void*)p->XN, (void*)p->AO, (void*)p->HB, (void*)p->HB2, (void*)p->QKV, (void*)p->ATT, (void*)p->seqpos, (void*)p->amax, d.dim, d.hidden, ctx->q_dim, d.ctx);
        GL3_HIP(hipFuncSetAttribute((const void*)gemm_f16_mfma_kernel<EPI_STORE>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * F16G_STAGE));
        GL3_HIP(hipFuncSetAttribute((const void*)gemm_f16_mfma_kernel<EPI_RESID>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * F16G_STAGE));
        GL3_HIP(hipFuncSetAttribute((const void*)gemm_f16_mfma_v512_kernel<EPI_STORE>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * F16G_STAGE));
        GL3_HIP(hipFuncSetAttribute((const void*)gemm_f16_mfma_v512_kernel<EPI_RESID>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * F16G_STAGE));
        GL3_HIP(hipFuncSetAttribute((const void*)gemm_vlq_kernel<WT_Q4_0, EPI_STORE>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * vlq_stage_floats<WT_Q4_0>() * 4));
        GL3_HIP(hipFuncSetAttribute((const void*)gemm_vlq_kernel<WT_Q4_0, EPI_RESID>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * vlq_stage_floats<WT_Q4_0>() * 4));
        GL3_HIP(hipFuncSetAttribute((const void*)gemm_vlq_kernel<WT_Q8_0, EPI_STORE>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * vlq_stage_floats<WT_Q8_0>() * 4));
        GL3_HIP(hipFuncSetAttribute((const void*)gemm_vlq_kernel<WT_Q8_0, EPI_RESID>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * vlq_stage_floats<WT_Q8_0>() * 4));
#define GL3_VQM_ATTR(WT_, EPI_, OCC_) GL3_HIP(hipFuncSetAttribute((const void*)gemm_vlq_mfma_kernel<WT_, EPI_, OCC_>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * VQM_STAGE_FLOATS * 4))
        GL3_VQM_ATTR(WT_Q4_0, EPI_STORE, 2); GL3_VQM_ATTR(WT_Q4_0, EPI_RESID, 2); GL3_VQM_ATTR(WT_Q4_0, EPI_STORE, 4); GL3_VQM_ATTR(WT_Q4_0, EPI_RESID, 4);
        GL3_VQM_ATTR(WT_Q8_0, EPI_STORE, 2); GL3_VQM_ATTR(WT_Q8_0, EPI_RESID, 2); GL3_VQM_ATTR(WT_Q8_0, EPI_STORE, 4); GL3_VQM_ATTR(WT_Q8_0, EPI_RESID, 4);
#undef GL3_VQM_ATTR
        return GL3_OK;
    }
    p->maxk = d.hidden > ctx->q_dim ? d.hidden : ctx->q_dim;
    if (d.dim > p->maxk) p->maxk = d.dim;
    p->maxk = (p->maxk + 127) & ~127;
    const size_t MQ = M < BD_TS_MAX ? BD_TS_MAX : M;      // the small-batch operand layout (bd_tslots) always spans its 32 / 64 token slots
    const size_t MQP = (MQ + 127) & ~(size_t)127;      // token slots of the chunk-major layouts (whole 128-token GEMM tiles)
    // pf_gemm3_kernel's LDS-DMA reads whole K stages: both chunk-major operands carry four blocks (one stage) beyond maxk, zeroed once here
    const size_t xq_bytes = MQP * (p->maxk + 4 * 32) + GL3_TAIL_PAD;
    const size_t xp_bytes = MQP * (p->maxk / 32 + 4) * 32 + GL3_TAIL_PAD;
    const size_t xs_bytes = MQ * (p->maxk / 32) * 4;
    GL3_HIP(hipMalloc((void**)&p->XQ, xq_bytes));
    GL3_HIP(hipMalloc((void**)&p->XS, xs_bytes + GL3_TAIL_PAD));
    p->xp_tok = (int)MQP;
    GL3_HIP(hipMalloc((void**)&p->XP, xp_bytes));
    GL3_HIP(hipMemsetAsync(p->XP, 0, xp_bytes, ctx->stream));
    if (M > 64 && d.tp_size == 1) {
        GL3_HIP(hipMalloc((void**)&p->XQh, xq_bytes));
        GL3_HIP(hipMalloc((void**)&p->XPh, xp_bytes));
        GL3_HIP(hipMemsetAsync(p->XQh, 0, xq_bytes, ctx->stream));
        GL3_HIP(hipMemsetAsync(p->XPh, 0, xp_bytes, ctx->stream));
    }
    GL3_HIP(hipMalloc((void**)&p->XQb, (size_t)BD_TS_MAX * p->maxk + GL3_TAIL_PAD));
    GL3_HIP(hipMalloc((void**)&p->XSb, (size_t)BD_TS_MAX * (p->maxk / 32) * 4 + GL3_TAIL_PAD));
    GL3_HIP(hipMemsetAsync(p->XQb, 0, (size_t)BD_TS_MAX * p->maxk, ctx->stream));
    GL3_HIP(hipMemsetAsync(p->XSb, 0, (size_t)BD_TS_MAX * (p->maxk / 32) * 4, ctx->stream));
    GL3_HIP(hipMemsetAsync(p->XQ, 0, xq_bytes, ctx->stream));
    GL3_HIP(hipMemsetAsync(p->XS, 0, xs_bytes, ctx->stream));
    GL3_HIP(gl3_gemm3_allow_lds());
    if (d.arch == GL3_ARCH_QWEN2MOE) {
        auto& m = p->moe;
        const size_t E = d.n_experts, K = d.n_experts_used, S = M * K;
        GL3_HIP(hipMalloc((void**)&m.logits, M * E * 4));
        GL3_HIP(hipMalloc((void**)&m.w, M * (K + 1) * 4));
        GL3_HIP(hipMalloc((void**)&m.sel, S * sizeof(int)));
        GL3_HIP(hipMalloc((void**)&m.ticket, M * sizeof(int)));
        GL3_HIP(hipMemsetAsync(m.ticket, 0, M * sizeof(int), ctx->stream));
        GL3_HIP(hipMalloc((void**)&m.slot_tok, S * sizeof(int)));
        GL3_HIP(hipMalloc((void**)&m.slot_dst, S * sizeof(int)));
        GL3_HIP(hipMalloc((void**)&m.tab, (size_t)(4 + 4 * moe_group_max_entries((int)M, (int)K, (int)E)) * sizeof(int)));
        GL3_HIP(hipMalloc((void**)&m.HB, S * d.moe_hidden * 4));
        GL3_HIP(hipMalloc((void**)&m.Y, M * (K + 1) * d.dim * 4));
        // XQ2 / XS2 operands with a run-time slot count: [ceil(k / 128) tiles + the ring's read-ahead][ts slots] x (128 B | 4 floats).
        // The rings of bdw_gemm_kernel read up to 8 tiles past the end unguarded, which here is more than GL3_TAIL_PAD: own slack.
        auto operand = [&](uint8_t** xq, float** xs, int k, int ts) -> hipError_t {
            const size_t tiles = (size_t)(k + 127) / 128 + 9;
            hipError_t e = hipMalloc((void**)xq, tiles * ts * 128);
            if (e == hipSuccess) e = hipMalloc((void**)xs, tiles * ts * 16);
            if (e == hipSuccess) e = hipMemsetAsync(*xq, 0, tiles * ts * 128, ctx->stream);
            if (e == hipSuccess) e = hipMemsetAsync(*xs, 0, tiles * ts * 16, ctx->stream);
            return e;
        };
        m.ts_x = (int)((M + 15) & ~(size_t)15);
        m.ts_h = (int)((S + 15) & ~(size_t)15);
        if (M > BD_TS_MAX) GL3_HIP(operand(&m.XQx, &m.XSx, d.dim, m.ts_x));
        GL3_HIP(operand(&m.XQh, &m.XSh, d.moe_hidden, m.ts_h));
        GL3_HIP(hipFuncSetAttribute((const void*)moe_router_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    }
    return GL3_OK;
}

void gl3_prefill_free(gl3_ctx* ctx) {
    gl3_prefill_state* p = ctx->pf;
    if (!p) return;
    for (auto ge : p->step_graphs) if (ge) hipGraphExecDestroy(ge);
    auto f = [](void* q) { if (q) hipFree(q); };
    f(p->tokens); f(p->XQ); f(p->XS); f(p->XP); f(p->XQh); f(p->XPh); f(p->XQb); f(p->XSb); f(p->QKV); f(p->ATT); f(p->TMX); f(p->SUMS); f(p->seqpos); f(p->tiles); f(p->deep); f(p->deep_rows); f(p->out_rows); f(p->XG); f(p->amax); f(p->amx_v); f(p->amx_i); f(p->XN); f(p->HB2);
    if (!p->in_arena) { f(p->X); f(p->AO); f(p->HB); f(p->LOGITS); }
    auto& m = p->moe;
    f(m.logits); f(m.w); f(m.sel); f(m.ticket); f(m.slot_tok); f(m.slot_dst); f(m.tab); f(m.HB); f(m.Y); f(m.XQx); f(m.XSx); f(m.XQh); f(m.XSh);
    delete p;
    ctx->pf = nullptr;
}

// bd_tslots(n) (gl3_bd_gemm.h): token slots of the XQ / XS operand layout when a step of n tokens runs on the wave-owned small-batch GEMM
// (bdw_gemm_kernel: n <= 64), 0 for a larger step.
// The one fact that fixes a step's activation layout: more than 64 tokens run on pf_gemm3_kernel / pf_gemm3t_kernel, which read the
// chunk-major int8 operand XQ[k / 16][token slot][16 B] and the scale operands XP.  Every producer of a GEMM operand (the quantiser,
// the attention and gate + up epilogues that quantise their own output) and launch_gemm ask here, so they cannot disagree.
static bool pf_chunk_major(int n) { return bd_tslots(n) == 0; }

// A/B switch of the fused producers, asked by the attention dispatch and both feed-forward blocks: GL3_NO_FUSED_QUANT=1 keeps the separate quantise launches
static bool pf_fused_quant_off() { static const bool off = env_flag("GL3_NO_FUSED_QUANT", false); return off; }

// The shape of one batched step: built once by its entry point, read by the layers, the attention dispatch and pf_fused_decode.
struct PfStep {
    int n;              // rows (tokens) of the step
    int max_pos;        // largest position of the step
    int one_seq;        // >= 0: all n rows belong to that sequence at consecutive positions ending at max_pos (prefill); -1: rows of many sequences
    int ntab;           // records of the attention tile table in p->tiles (the shallow tiles); 0 unless a mixed step has a run of several rows
    int ndeep;          // records of the deep table in p->deep: rows past the one-launch table form's depth, on the long-context trio
    int deep_rows;      // step rows of the deep records (p->deep_rows)
    int tab_max_pos;    // last position of the deepest shallow tile (ndeep > 0 only: sizes the one-launch kernels' score rows)
    bool runs() const { return ntab + ndeep > 0; }      // a mixed step with a run of several rows
};

// A static-batched decode step whose deepest row is at max_pos runs the one-launch attention (attn_head_kernel).  Asked by the attention
// dispatch, by the operand hand-over behind it and by the graph capture of the step (only such a step has nothing position-dependent
// baked in: the three-kernel attention sizes its scores grid by the deepest row), so they cannot disagree.
// A mixed step with a run of several rows (st.runs()) never does: attn_head_kernel writes a row's K / V in the launch that reads it, and a
// later row of the same run would race with that write.
static bool pf_fused_decode(const gl3_ctx* ctx, const PfStep& st) {
    static const bool bd_attn_off = env_flag("GL3_NO_FUSED_BD_ATTN", false);      // A/B switch: =1 the three-kernel attention of static-batched decode
    return ctx->fused_attn_ok && st.max_pos < AF_MAXN && !bd_attn_off && !st.runs();
}


// Where a quantise launch writes: an int8 operand set in the layout its slot count names (tslots 0: chunk-major with the scales in XP), or,
// for the f32 modes, plain f32 rows in XS.
struct PfOperand {
    uint8_t* XQ; float* XS;      // int8 blocks and their scales; f32 modes: XQ null, XS = the f32 destination rows (XN)
    int maxk, tslots; uint8_t* XP; int xp_tok;      // 0 / null for the f32 modes
};
static PfOperand pf_operand(const gl3_prefill_state* p, int n) { return {p->XQ, p->XS, p->maxk, bd_tslots(n), p->XP, p->xp_tok}; }      // the next GEMM's, for a step of n tokens
static PfOperand pf_operand_f32(const gl3_prefill_state* p) { return {nullptr, p->XN, 0, 0, nullptr, 0}; }

// The one launch of pf_norm_quant_kernel: `rows` rows of k elements of src (rank-chunked, chunk width cc) -> dst.  The NORM modes take one
// workgroup per row with the row in LDS, the PLAIN modes one per (row, 1024 elements) and no LDS; norm_w is null for the PLAIN modes.
template <int MODE>
static void pf_quant(gl3_ctx* ctx, const float* src, int k, int cc, const float* norm_w, int rows, const PfOperand& dst) {
    constexpr bool NORM = MODE == PQ_NORM || MODE == PQ_NORM_F32;
    hipLaunchKernelGGL((pf_norm_quant_kernel<MODE>), NORM ? dim3(rows) : dim3(rows, (k / 4 + 255) / 256), dim3(256), NORM ? nq_smem(k) : 0, ctx->stream,
                       src, k, cc, norm_w, NORM ? ctx->d.rms_eps : 0.f, dst.XQ, dst.XS, dst.maxk, dst.tslots, (uint2*)dst.XP, dst.xp_tok);
}

template <int EPI>
static void launch_gemm(gl3_ctx* ctx, const Q8Mat& w, const Q8Mat* w2, int ntok, float* out, int out_stride, float out_scale = 1.0f,
                        bool second_operand = false, bool quantised_out = false) {
    gl3_prefill_state* p = ctx->pf;
    GemmArgs a{};
    a.w = w.w; a.w2 = w2 ? w2->w : nullptr; a.rows = w.rows; a.ng = w.ng; a.nb = w.k / 32;
    a.XQ = second_operand ? p->XQb : p->XQ; a.XS = second_operand ? p->XSb : p->XS;
    a.maxk = p->maxk; a.ntok = ntok; a.out = out; a.out_stride = out_stride; a.out_scale = out_scale;
    a.XQo = p->XQb; a.XSo = p->XSb;
    a.XP = p->XP; a.xp_tok = p->xp_tok;
    if (pf_chunk_major(ntok)) {      // > 64 tokens: pf_gemm3_kernel / pf_gemm3t_kernel, tiling by matrix shape (gl3_prefill_gemm3.hip)
        if (quantised_out) { a.XQo = p->XQh; a.XPo = p->XPh; }          // gate + up: hb as the down projection's operand (tall tiling, one rank)
        if (second_operand) { a.XQ = p->XQh; a.XP = p->XPh; }            // down: reads it
        gl3_gemm3_launch(EPI, a, w.rows, ntok, ctx->stream);
        return;
    }
    // static-batched decode / small chunks: one wavefront per (16-row strip, 16 tokens), all of K
    const BdGemmPlan pl = bd_gemm_plan(EPI, w.rows, w.k, ntok, quantised_out);      // quantised output: two strips per workgroup
    a.tslots = pl.tslots;
    const dim3 grid(pl.grid), block(pl.threads);
#define GL3_BDW(TS_) \
    do { \
        if constexpr (EPI == EPI_SWIGLU) { \
            if (pl.qout) hipLaunchKernelGGL((bdw_gemm_kernel<EPI, 4, 2, true, TS_>), grid, block, 0, ctx->stream, a); \
            else hipLaunchKernelGGL((bdw_gemm_kernel<EPI, 4, 2, false, TS_>), grid, block, 0, ctx->stream, a); \
        } else hipLaunchKernelGGL((bdw_gemm_kernel<EPI, 8, 2, false, TS_>), grid, block, 0, ctx->stream, a); \
    } while (0)
    if (pl.tslots == BD_TS) GL3_BDW(BD_TS); else GL3_BDW(BD_TS_MAX);
#undef GL3_BDW
}

int32_t gl3_debug_bd_gemm_plan(int32_t epi, int32_t rows, int32_t k, int32_t ntok, int32_t quantised_out, int32_t wg, int32_t out[12]) {
    if (!out || rows < 1 || k < 32 || k % 32 || ntok < 1 || (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_SWIGLU)) return GL3_E_ARG;
    const BdGemmPlan p = bd_gemm_plan(epi, rows, k, ntok, quantised_out != 0);
    out[0] = p.tslots; out[1] = p.DA; out[2] = p.qout; out[3] = p.threads; out[4] = p.ntt; out[5] = p.units; out[6] = p.grid;
    out[7] = p.ntiles; out[8] = p.trips; out[9] = p.partial;
    out[10] = out[11] = -1;                              // workgroup wg: its unit and token tile; -1: no such workgroup, or it exits
    if (p.tslots && wg >= 0 && wg < p.grid) {
        const int unit = bdw_place_unit((unsigned)wg, p.ntt);
        if (unit < p.units) { out[10] = unit; out[11] = bdw_place_tile((unsigned)wg, p.ntt); }
    }
    return GL3_OK;
}

// The routed experts of a Qwen2-MoE step: one launch over (tile-table entry, strip of the entry's expert) — bdw_gemm_kernel<.., GRP>.
// w / w2 = the stacked expert tensors, rows = rows of one expert; XQ / XS = the operand in the XQ2 / XS2 layout with ts token slots;
// gtok / gdst as in GemmArgs.  The grid covers the bound on the table's entries for n tokens; surplus workgroups exit.
template <int EPI>
static void launch_gemm_grouped(gl3_ctx* ctx, const Q8Mat& w, const Q8Mat* w2, int rows, int n, const uint8_t* XQ, const float* XS, int ts,
                                const int* gtok, const int* gdst, float* out, int out_stride) {
    gl3_prefill_state* p = ctx->pf;
    GemmArgs a{};
    a.w = w.w; a.w2 = w2 ? w2->w : nullptr; a.rows = rows; a.ng = w.ng; a.nb = w.k / 32;
    a.XQ = XQ; a.XS = XS; a.tslots = ts; a.ntok = n; a.out = out; a.out_stride = out_stride; a.out_scale = 1.0f;
    a.gtab = p->moe.tab; a.gtok = gtok; a.gdst = gdst; a.gspe = rows / 16;
    const dim3 grid((unsigned)moe_group_max_entries(n, ctx->d.n_experts_used, ctx->d.n_experts) * a.gspe);
    if constexpr (EPI == EPI_SWIGLU) hipLaunchKernelGGL((bdw_gemm_kernel<EPI, 4, 2, false, BD_TS, true>), grid, dim3(64), 0, ctx->stream, a);
    else hipLaunchKernelGGL((bdw_gemm_kernel<EPI, 8, 2, false, BD_TS, true>), grid, dim3(64), 0, ctx->stream, a);
}

// A head size / head-slot count that a prefill attention kernel takes as a template argument: f(std::integral_constant<int, ...>{}).  MIN_HS = 64: the
// kernels with their products on the matrix pipe, which exist for head sizes 128 and 64 only (their callers have checked the shape).  HS96: the VALU
// long-context kernels (pf_scores_pk_kernel, pf_scores_tiled_kernel, pf_pv_ring_kernel), the only tiled kernels instantiated for head size 96.
template <int MIN_HS, bool HS96 = false, class F>
static inline void pf_head_dispatch(int hs, F&& f) {
    if (hs == 128) f(std::integral_constant<int, 128>{});
    else if (hs == 64) f(std::integral_constant<int, 64>{});
    else if (HS96 && hs == 96) { if constexpr (HS96) f(std::integral_constant<int, 96>{}); }
    else if constexpr (MIN_HS <= 32) f(std::integral_constant<int, 32>{});
}
template <class F>
static inline void pf_kvmul_dispatch(int slots, F&& f) {      // pf_scores_pk_kernel: 4, 2 or 1 head slots per workgroup
    if (slots == 4) f(std::integral_constant<int, 4>{});
    else if (slots == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 1>{});
}

// The conditions that pf_attention and the split limit of a plan's mixed steps (pf_tab_max_pos) both ask, so they cannot disagree.  The
// switches are read once per process.
static bool pf_sw_fused_off() { static const bool v = getenv("GL3_PF_FUSED_ATTN") && atoi(getenv("GL3_PF_FUSED_ATTN")) == 0; return v; }
static bool pf_sw_v1_only() { static const bool v = env_flag("GL3_PF_FUSED_V1", false); return v; }
// pf_softmax_rows_kernel (the long-context trio's softmax) reads 16-byte pieces of 64-timestep tiles of the score rows; a plan without it has
// the one-launch kernels and the per-row pair
static bool pf_rows_softmax(const gl3_ctx* ctx) { return ctx->d.ctx % 4 == 0 && ctx->d.ctx >= 64; }
// A workgroup of the tiled kernels serves a head group (HeadGroup, gl3_prefill_attn.h): pf_group_size(kvMul) head slots, pf_head_groups(kvMul) groups per
// kv head.  Every LDS size and fit below is asked with the group size: a grouped shape has the limits of kvMul 4 at its head size.
static int pf_group_size(int kvmul) { return std::min(kvmul, 4); }
static int pf_head_groups(int kvmul) { const int g = pf_group_size(kvmul); return (kvmul + g - 1) / g; }
// Shapes the tiled kernels exist for.  kvMul <= 4 at head size 32 / 64 / 128: as ever.  kvMul 5 - 16 (head groups) and head size 96 (the VALU
// long-context kernels only; the group is orthogonal to the head size, so 96 is served above kvMul 4 too): with pf_softmax_rows_kernel and without
// the switch whose kernel knows neither (GL3_PF_FUSED_V1=1: pf_attn_fused_kernel) — there they keep the per-row pair.
static bool pf_tiled_shape(int hs, int kvmul, bool rows_softmax) {
    if (kvmul <= 4 && (hs == 32 || hs == 64 || hs == 128)) return true;
    return kvmul <= 16 && (hs == 32 || hs == 64 || hs == 96 || hs == 128) && rows_softmax && !pf_sw_v1_only();
}
static int pf_fa_sstride(int max_pos) { return ((max_pos + 1 + 63) & ~63) + 4; }      // floats of a score row of the one-launch kernels whose deepest row is at max_pos
// r4: one launch for scores + softmax + weighted V sum when a tile's score rows fit LDS (GL3_PF_FUSED_ATTN=0: the three kernels)
// (group = head slots of a workgroup, pf_group_size; no one-launch kernel at head size 96)
static bool pf_one_launch_fits(int hs, int group, int sstride) {
    return !pf_sw_fused_off() && hs != 96 && 64 * (hs / 4) <= 8 * 64 * group && fa_smem_bytes(hs, group, sstride) <= PF_ATTN_LDS_MAX;      // 8 float4 per thread stage a tile
}
// the table form exists for pf_attn_fused3_kernel / pf_attn_fused2_kernel only: with fused2's rows fitting, one of the two is what the dispatch picks
static bool pf_tab_fits(int hs, int group, int sstride) {
    return pf_one_launch_fits(hs, group, sstride) && !pf_sw_v1_only() && fa2_smem_bytes(hs, group, sstride) <= PF_ATTN_LDS_MAX;
}
// fused_max_pos of a plan's mixed steps (batch_plan_split): the largest last position a tile may have in the one-launch table form, -1 for
// a tiled shape without one.  INT_MAX — no split, the dispatch of a step is by its deepest row as before — where the long-context trio
// cannot take the deep rows: shapes without tiled kernels, plans without pf_softmax_rows_kernel.
// GL3_PF_TAB_MAXPOS=<p> (diagnostic) lowers the limit to min(own, p), so that a short-context model exercises the split.
static int pf_tab_max_pos(const gl3_ctx* ctx) {
    static const char* env = getenv("GL3_PF_TAB_MAXPOS");
    const int hs = ctx->d.head_size, kvmul = ctx->d.n_heads / ctx->d.n_kv_heads, group = pf_group_size(kvmul);
    if (!pf_rows_softmax(ctx) || !pf_tiled_shape(hs, kvmul, true)) return INT_MAX;
    int fm = -1;
    for (int k = 1; 64 * (k - 1) < ctx->d.ctx && pf_tab_fits(hs, group, pf_fa_sstride(64 * k - 1)); ++k) fm = 64 * k - 1;      // score rows grow by 64 positions
    if (env && *env) fm = std::min(fm, atoi(env));
    return fm;
}

// RoPE + KV write + attention of layer l for the n tokens whose raw q | k | v rows are in p->QKV -> AOr (this rank's chunk of the
// attention output).  fuse_q: static-batched decode on one rank writes the output as the wo projection's int8 operand instead.
// returns true when the attention output was written as the wo projection's int8 operand (no quantise launch needed)
// A mixed step with runs of several rows (st.runs(), one_seq < 0): after the one RoPE + KV launch every K / V row of the step is in the
// caches.  Its shallow tiles (st.ntab records in p->tiles) take the run-table form of the one-launch kernels, its deep rows (st.ndeep records
// in p->deep, rows past the depth at which a tile's score rows fit LDS) the run-table form of the long-context trio; a step with both writes
// its output as f32 and the caller's quantise launch serves all rows.  Shapes without tiled kernels and plans without pf_softmax_rows_kernel
// are not split (pf_tab_max_pos): there the whole step takes the one-launch kernels (a mixed step: their table form) or, failing that, the
// per-row pair.
// Every return notes the step's rows by the form that served them (gl3_get_attn_rows).
static bool pf_attention(gl3_ctx* ctx, int l, const PfStep& st, float* AOr, bool fuse_q) {
    // A/B switches, read once at the first call, whichever branch it takes (they are set for the life of the process; nothing sets one
    // after the first step); each says what it turns off where it is used.  The default-on ones keep the getenv / atoi form: set to the
    // empty string it turns the feature off, where env_flag(x, true) would leave it on
    static const bool v1_only = pf_sw_v1_only();      // (GL3_PF_FUSED_ATTN, GL3_PF_FUSED_V1: above, shared with pf_tab_max_pos, which reads GL3_PF_TAB_MAXPOS)
    static const bool qao_off = getenv("GL3_PF_ATTN_QOUT") && atoi(getenv("GL3_PF_ATTN_QOUT")) == 0;
    static const bool mfma_off = getenv("GL3_PF_FUSED_MFMA") && atoi(getenv("GL3_PF_FUSED_MFMA")) == 0;
    static const bool pk_off = getenv("GL3_PF_SCORES_PK") && atoi(getenv("GL3_PF_SCORES_PK")) == 0;
    static const bool scm_off = getenv("GL3_PF_SCORES_MFMA") && atoi(getenv("GL3_PF_SCORES_MFMA")) == 0;
    static const int scm_split = getenv("GL3_SCM_SPLIT") ? atoi(getenv("GL3_SCM_SPLIT")) : SCM_SPLIT;      // workgroups that share a (kv head, token tile)'s K tiles
    static const bool pvm_off = getenv("GL3_PF_PV_MFMA") && atoi(getenv("GL3_PF_PV_MFMA")) == 0;
    const int n = st.n, max_pos = st.max_pos, one_seq = st.one_seq, ntab = st.ntab, ndeep = st.ndeep;
    const bool runs = st.runs();                          // the run-table forms
    gl3_prefill_state* p = ctx->pf;
    auto note_rows = [p](int head, int one, int trio, int pair) { p->attn_rows[0] = head; p->attn_rows[1] = one; p->attn_rows[2] = trio; p->attn_rows[3] = pair; p->attn_rows_set = true; };
    const gl3_model_desc& d = ctx->d;
    hipStream_t s = ctx->stream;
    gl3_layer& L = ctx->layers[l];
    const int32_t* seq = p->seqpos;
    const int32_t* pos = p->seqpos + p->max_batch;
    const int kvmul = d.n_heads / d.n_kv_heads;
    const int H = ctx->heads_l, KVH = ctx->kv_heads_l, qd = ctx->q_dim_l, kvd = ctx->kv_dim_l;
    const int qkv_dim = qd + 2 * kvd;
    const size_t kv_layer = (size_t)d.ctx * kvd;
    // one workgroup per (kv head, token) serves the kv head's whole group of query heads when its LDS image fits
    const int bd_group = (kvmul <= 8 && attn_head_admits(d.head_size, kvmul)) ? kvmul : 1;
    const bool fused_decode = pf_fused_decode(ctx, st);
    RopeArgs ra{};
    ra.QKV = p->QKV; ra.qkv_stride = qkv_dim; ra.kcache = ctx->kcache + l * kv_layer; ra.vcache = ctx->vcache + l * kv_layer;
    ra.cr = ctx->rope_cr; ra.ci = ctx->rope_ci; ra.qnorm = L.qnorm; ra.knorm = L.knorm; ra.bq = L.bq; ra.bk = L.bk; ra.bv = L.bv; ra.n_heads = H;
    ra.n_kv_heads = KVH; ra.hs = d.head_size; ra.q_dim = qd; ra.kv_dim = kvd;
    ra.arch = ctx->rope_arch; ra.eps = d.rms_eps; ra.seq = seq; ra.pos = pos; ra.seq_stride = ctx->kv_seq_stride;
    PfAttnArgs aa{};
    aa.Q = p->QKV; aa.q_stride = qkv_dim; aa.kcache = ra.kcache; aa.vcache = ra.vcache; aa.att = p->ATT; aa.out = AOr;
    aa.out_stride = qd; aa.n_heads = H; aa.n_kv_heads = KVH; aa.hs = d.head_size; aa.kv_dim = kvd;
    aa.ctx = d.ctx; aa.seq = seq; aa.pos = pos; aa.seq_stride = ctx->kv_seq_stride; aa.att_mul = ctx->att_mul;
    const int nsplit = (max_pos + 1 + ATT_TT - 1) / ATT_TT;
    const int hs = d.head_size;
    if (one_seq < 0 && fused_decode) {
        // static-batched decode at positions < AF_MAXN: RoPE + KV write + scores + softmax + weighted V sum of every
        // (token, head) in ONE launch (attn_head_kernel, grid = heads x tokens) instead of three per-token-grid kernels
        AttnArgs ha{};
        gl3_attn_layer_args(ctx, l, ha);
        ha.qkv = p->QKV; ha.qkv_stride = qkv_dim; ha.dyn = ctx->dyn; ha.att = nullptr; ha.xb = AOr; ha.xb_stride = qd;
        ha.seqv = seq; ha.posv = pos; ha.seq_stride = ctx->kv_seq_stride;
        ha.group = bd_group;
        if (fuse_q) { ha.xq_out = p->XQ; ha.xs_out = p->XS; ha.xq_slots = bd_tslots(n); }
        attn_head_dispatch(hs, [&](auto kern) { hipLaunchKernelGGL(kern, dim3(H / bd_group, n), dim3(256), attn_head_smem(hs, bd_group), s, ha); });
        note_rows(n, 0, 0, 0);
        return fuse_q;
    }
    hipLaunchKernelGGL(pf_rope_kv_kernel, dim3(H + KVH, n), dim3(64), 0, s, ra);
    const bool rows_softmax = pf_rows_softmax(ctx);
    const bool tiled = (one_seq >= 0 || runs) && pf_tiled_shape(hs, kvmul, rows_softmax);
    const int group = pf_group_size(kvmul), NG = pf_head_groups(kvmul);      // head slots of a tiled workgroup, head groups per kv head (kvMul <= 4: kvMul, 1)
    const bool mfma_shape = group == 4 && (hs == 128 || hs == 64);      // the kernels with their products on the matrix pipe
    const int fa_sstride = pf_fa_sstride(ndeep ? st.tab_max_pos : max_pos);      // sized by the deepest row the one-launch kernels serve: of the step, or of its shallow tiles
    // (a grouped shape has no pf_attn_fused_kernel form: its one-launch kernels are those of the table form, fused3 / fused2)
    const bool one_launch = NG > 1 ? pf_tab_fits(hs, group, fa_sstride) : pf_one_launch_fits(hs, group, fa_sstride);
    const bool tab_ok = ntab > 0 && tiled && pf_tab_fits(hs, group, fa_sstride);
    // several sequences, a shape the tiled kernels do not have, or rows past the one-launch kernels with no trio to take them (a table the
    // one-launch kernels cannot serve, a plan without pf_softmax_rows_kernel): the per-token pair
    if (!tiled || (ntab > 0 && !tab_ok) || (!rows_softmax && !one_launch)) {
        const size_t sm1 = ((size_t)kvmul * d.head_size + (size_t)ATT_TT * (d.head_size + 1)) * 4;
        hipLaunchKernelGGL(pf_attn_scores_kernel, dim3(nsplit, KVH, n), dim3(64 * kvmul), sm1, s, aa);
        aa.win = ctx->attn_win;
        hipLaunchKernelGGL(pf_attn_softmax_pv_kernel, dim3(H * ((d.head_size + 63) / 64), n), dim3(64), (size_t)ctx->attn_win * 4 + 16, s, aa);
        note_rows(0, 0, 0, n);
        return false;
    }
    const int pos0 = max_pos + 1 - n;      // one sequence: token b of the chunk sits at position pos0 + b
    const float* kc1 = aa.kcache + (size_t)(runs ? 0 : one_seq) * ctx->kv_seq_stride;      // table forms: the tile's record names its sequence
    const float* vc1 = aa.vcache + (size_t)(runs ? 0 : one_seq) * ctx->kv_seq_stride;
    const size_t sst = ctx->kv_seq_stride;
    if (one_launch && (ndeep == 0 || ntab > 0)) {
        const dim3 grid(KVH * (runs ? ntab : (n + FA_TB - 1) / FA_TB), NG);
        // r6: > 64 tokens on one rank with head size 128: the output is written quantised for the wo GEMM (pf_gemm3_kernel's operand layout).
        // Not in a step that also has deep tiles: the trio writes f32 rows, and the caller's quantise launch serves all rows of the step
        const bool qao = ndeep == 0 && !qao_off && hs == 128 && pf_chunk_major(n) && d.tp_size == 1 && p->XP && !pf_fused_quant_off();
        uint8_t* xqo = qao ? p->XQ : nullptr;
        uint4* xpo = qao ? reinterpret_cast<uint4*>(p->XP) : nullptr;
        // r6: products of both phases on the matrix pipe (pf_attn_fused3_kernel); GL3_PF_FUSED_MFMA=0: the VALU kernels.  Else packed-f32 scores + pinned
        // weighted V sum (pf_attn_fused2_kernel) while its 16 KB of query rows still fit; GL3_PF_FUSED_V1=1: the r4 kernel
        const size_t sms = fa_smem_bytes(hs, group, fa_sstride), sms2 = fa2_smem_bytes(hs, group, fa_sstride), sms3 = fa3_smem_bytes(hs, fa_sstride);
        if (!mfma_off && !v1_only && mfma_shape && sms3 <= PF_ATTN_LDS_MAX)
            pf_head_dispatch<64>(hs, [&](auto hc) {
                constexpr int HS_ = decltype(hc)::value;
                if (runs) hipLaunchKernelGGL((pf_attn_fused3_kernel<HS_, true>), grid, dim3(512), sms3, s, aa.Q, aa.q_stride, kc1, vc1, aa.out, aa.out_stride,
                                             KVH, kvmul, aa.kv_dim, 0, n, aa.att_mul, fa_sstride, xqo, xpo, p->xp_tok, p->tiles, sst);
                else hipLaunchKernelGGL((pf_attn_fused3_kernel<HS_>), grid, dim3(512), sms3, s, aa.Q, aa.q_stride, kc1, vc1, aa.out, aa.out_stride,
                                        KVH, kvmul, aa.kv_dim, pos0, n, aa.att_mul, fa_sstride, xqo, xpo, p->xp_tok, (const int4*)nullptr, (size_t)0); });
        else if (!v1_only && sms2 <= PF_ATTN_LDS_MAX)
            pf_head_dispatch<32>(hs, [&](auto hc) {
                constexpr int HS_ = decltype(hc)::value;
                if (runs) hipLaunchKernelGGL((pf_attn_fused2_kernel<HS_, true>), grid, dim3(128 * group), sms2, s, aa.Q, aa.q_stride, kc1, vc1, aa.out, aa.out_stride,
                                             KVH, group, kvmul, aa.kv_dim, 0, n, aa.att_mul, fa_sstride, xqo, xpo, p->xp_tok, p->tiles, sst);
                else hipLaunchKernelGGL((pf_attn_fused2_kernel<HS_>), grid, dim3(128 * group), sms2, s, aa.Q, aa.q_stride, kc1, vc1, aa.out, aa.out_stride,
                                        KVH, group, kvmul, aa.kv_dim, pos0, n, aa.att_mul, fa_sstride, xqo, xpo, p->xp_tok, (const int4*)nullptr, (size_t)0); });
        else
            pf_head_dispatch<32>(hs, [&](auto hc) {
                hipLaunchKernelGGL((pf_attn_fused_kernel<decltype(hc)::value>), grid, dim3(128 * kvmul), sms, s, aa.Q, aa.q_stride, kc1, vc1, aa.out, aa.out_stride,
                                   KVH, kvmul, aa.kv_dim, pos0, n, aa.att_mul, fa_sstride, xqo, xpo, p->xp_tok); });
        if (ndeep == 0) { note_rows(0, n, 0, 0); return qao; }
    }
    // The long-context trio over score rows in HBM: one sequence's chunk in token tiles of 16 (weighted V sum: 32 on the ring kernel), or
    // (ndeep > 0) the deep records of a mixed step in the kernels' table forms, the deepest of which sizes the timestep grid
    const int4* dtab = p->deep;
    const int ntt = ndeep ? ndeep : (n + PA_TB - 1) / PA_TB;
    const dim3 g1(nsplit, KVH * NG, ntt), b1(64 * group);
    const bool pk = !pk_off && scores_pk_smem_bytes(hs, group) <= PF_ATTN_LDS_MAX && (group == 4 || group == 2 || group == 1);
    if (!scm_off && mfma_shape) {      // r6: products on the matrix pipe, query rows resident, K tiles prefetched
        const dim3 g(nsplit < scm_split ? nsplit : scm_split, KVH * NG, ndeep ? ndeep : (n + SCM_TB - 1) / SCM_TB);
        pf_head_dispatch<64>(hs, [&](auto hc) {
            constexpr int HS_ = decltype(hc)::value;
            if (ndeep) hipLaunchKernelGGL((pf_scores_mfma_kernel<HS_, true>), g, dim3(512), scores_mfma_smem_bytes(hs), s, aa.Q, aa.q_stride, kc1, aa.att, aa.n_heads,
                                          kvmul, aa.kv_dim, aa.ctx, 0, n, aa.att_mul, p->TMX, p->tmx_tiles, dtab, sst);
            else hipLaunchKernelGGL((pf_scores_mfma_kernel<HS_>), g, dim3(512), scores_mfma_smem_bytes(hs), s, aa.Q, aa.q_stride, kc1, aa.att, aa.n_heads,
                                    kvmul, aa.kv_dim, aa.ctx, pos0, n, aa.att_mul, p->TMX, p->tmx_tiles); });
    } else if (pk)
        pf_head_dispatch<32, true>(hs, [&](auto hc) { pf_kvmul_dispatch(group, [&](auto mc) {
            constexpr int HS_ = decltype(hc)::value, KVM_ = decltype(mc)::value;
            if (ndeep) hipLaunchKernelGGL((pf_scores_pk_kernel<HS_, KVM_, true>), g1, b1, scores_pk_smem_bytes(hs, group), s, aa.Q, aa.q_stride, kc1, aa.att,
                                          aa.n_heads, kvmul, aa.kv_dim, aa.ctx, 0, n, aa.att_mul, p->TMX, p->tmx_tiles, dtab, sst);
            else hipLaunchKernelGGL((pf_scores_pk_kernel<HS_, KVM_>), g1, b1, scores_pk_smem_bytes(hs, group), s, aa.Q, aa.q_stride, kc1, aa.att,
                                    aa.n_heads, kvmul, aa.kv_dim, aa.ctx, pos0, n, aa.att_mul, p->TMX, p->tmx_tiles); }); });
    else
        pf_head_dispatch<32, true>(hs, [&](auto hc) {
            constexpr int HS_ = decltype(hc)::value;
            if (ndeep) hipLaunchKernelGGL((pf_scores_tiled_kernel<HS_, true>), g1, b1, scores_tiled_smem_bytes(hs), s, aa.Q, aa.q_stride, kc1, aa.att,
                                          aa.n_heads, kvmul, aa.kv_dim, aa.ctx, 0, n, aa.att_mul, p->TMX, p->tmx_tiles, dtab, sst);
            else hipLaunchKernelGGL((pf_scores_tiled_kernel<HS_>), g1, b1, scores_tiled_smem_bytes(hs), s, aa.Q, aa.q_stride, kc1, aa.att,
                                    aa.n_heads, kvmul, aa.kv_dim, aa.ctx, pos0, n, aa.att_mul, p->TMX, p->tmx_tiles); });
    // r6: R rows per workgroup, the sums as R chains of one wavefront; at least one workgroup per CU when the chunk has the rows.
    // A split step: the deep rows only (a shallow row's ATT / TMX were not written in this step)
    const int rows = (ndeep ? st.deep_rows : n) * H;
    const int32_t* rlist = ndeep ? p->deep_rows : nullptr;
    const float* sums = p->SUMS;
    if (rows >= 64 * 256) hipLaunchKernelGGL((pf_softmax_rows_kernel<64>), dim3((rows + 63) / 64), dim3(576), 0, s, aa, rows, p->TMX, p->tmx_tiles, p->SUMS, rlist);
    else if (rows >= 32 * 256) hipLaunchKernelGGL((pf_softmax_rows_kernel<32>), dim3((rows + 31) / 32), dim3(576), 0, s, aa, rows, p->TMX, p->tmx_tiles, p->SUMS, rlist);
    else hipLaunchKernelGGL((pf_softmax_rows_kernel<16>), dim3((rows + 15) / 16), dim3(576), 0, s, aa, rows, p->TMX, p->tmx_tiles, p->SUMS, rlist);
    if (!pvm_off && mfma_shape)                         // r6: products on the matrix pipe (no uniform-address LDS reads)
        pf_head_dispatch<64>(hs, [&](auto hc) {
            constexpr int HS_ = decltype(hc)::value;
            if (ndeep) hipLaunchKernelGGL((pf_pv_mfma_kernel<HS_, true>), dim3(KVH * NG, ndeep), dim3(1024), pv_mfma_smem_bytes(hs), s, aa, 0, 0, n, sums, dtab);
            else hipLaunchKernelGGL((pf_pv_mfma_kernel<HS_>), dim3(KVH * NG, (n + PVM_TB - 1) / PVM_TB), dim3(1024), pv_mfma_smem_bytes(hs), s, aa, one_seq, pos0, n, sums); });
    else
        pf_head_dispatch<32, true>(hs, [&](auto hc) {
            constexpr int HS_ = decltype(hc)::value;
            if (ndeep) hipLaunchKernelGGL((pf_pv_ring_kernel<HS_, true>), dim3(H, ndeep), dim3(64 * PVR_NW), pv_ring_smem_bytes(hs), s, aa, 0, 0, n, sums, dtab);
            else hipLaunchKernelGGL((pf_pv_ring_kernel<HS_>), dim3(H, (n + PVR_TB - 1) / PVR_TB), dim3(64 * PVR_NW), pv_ring_smem_bytes(hs), s, aa, one_seq, pos0, n, sums); });
    if (ndeep) note_rows(0, n - st.deep_rows, st.deep_rows, 0);
    else note_rows(0, 0, n, 0);
    return false;
}

// Batched matmul of the f32-activation weight types (gl3_prefill_vl.h): out[b][row] (+)= dot(W[row], act[b]) in the Vector-API order.
// The switches of the choice are read once per process; vl_gemm_plan makes the choice (kernel, tiles, grid).
static const VlGemmSwitches& vl_gemm_switches() {
    static const VlGemmSwitches sw = [] {
        VlGemmSwitches x;
        x.mfma = env_flag("GL3_VLQ_MFMA", true);
        x.xcd_tokens = env_flag("GL3_VQM_XCD_TOKENS", true);
        x.occ2 = env_flag("GL3_VQM_OCC2", false);
        const char* v = getenv("GL3_VLQ_MFMA_MIN_TILES");
        if (v && *v && atoi(v) > 0) x.min_tiles = atoi(v);
        return x;
    }();
    return sw;
}

template <int EPI>
static void launch_gemm_vl(gl3_ctx* ctx, const Q8Mat& w, int ntok, const float* act, int act_stride, float* out, int out_stride, float out_scale = 1.0f) {
    const VlGemmSwitches& sw = vl_gemm_switches();
    const VlGemmPlan pl = vl_gemm_plan(w.fmt, (ctx->d.flags & GL3_FLAG_VECTOR_512) != 0, w.rows, ntok, sw);
    VlGemmArgs a{};
    a.w = w.w; a.rows = w.rows; a.k = w.k; a.X = act; a.x_stride = act_stride; a.ntok = ntok; a.out = out; a.out_stride = out_stride; a.out_scale = out_scale;
    a.nrt = pl.nrt; a.ntt = pl.ntt; a.xcd_tokens = pl.xcd_tokens;
    const dim3 g(pl.grid);
    switch (pl.kernel) {
    case VLG_F16_MFMA_V512:                              // 16 accumulator lanes: the same tiles, a wavefront pair per sub-tile
        hipLaunchKernelGGL((gemm_f16_mfma_v512_kernel<EPI>), g, dim3(512), 2 * F16G_STAGE, ctx->stream, a);
        break;
    case VLG_F16_MFMA:
        hipLaunchKernelGGL((gemm_f16_mfma_kernel<EPI>), g, dim3(256), 2 * F16G_STAGE, ctx->stream, a);
        break;
    case VLG_VLQ_MFMA: {
        // enough 64 x 64 tiles to fill the chip: products on the f32 matrix cores (gemm_vlq_mfma_kernel; 8B Q4_0 pp512 2.53 k -> 3.4 k
        // tok/s).  Fewer tiles (short chunks, the 4096-row projections at 128 tokens) keep the 16-token VALU kernel; GL3_VLQ_MFMA=0: always.
        const size_t sm = (size_t)2 * VQM_STAGE_FLOATS * 4;
        if (w.fmt == GL3_TYPE_Q4_0) {
            if (sw.occ2) hipLaunchKernelGGL((gemm_vlq_mfma_kernel<WT_Q4_0, EPI, 2>), g, dim3(512), sm, ctx->stream, a);
            else hipLaunchKernelGGL((gemm_vlq_mfma_kernel<WT_Q4_0, EPI, 4>), g, dim3(512), sm, ctx->stream, a);
        } else {
            if (sw.occ2) hipLaunchKernelGGL((gemm_vlq_mfma_kernel<WT_Q8_0, EPI, 2>), g, dim3(512), sm, ctx->stream, a);
            else hipLaunchKernelGGL((gemm_vlq_mfma_kernel<WT_Q8_0, EPI, 4>), g, dim3(512), sm, ctx->stream, a);
        }
        break;
    }
    default:
        if (w.fmt == GL3_TYPE_Q4_0) hipLaunchKernelGGL((gemm_vlq_kernel<WT_Q4_0, EPI>), g, dim3(256), 2 * vlq_stage_floats<WT_Q4_0>() * 4, ctx->stream, a);
        else hipLaunchKernelGGL((gemm_vlq_kernel<WT_Q8_0, EPI>), g, dim3(256), 2 * vlq_stage_floats<WT_Q8_0>() * 4, ctx->stream, a);
    }
}

int32_t gl3_debug_vl_gemm_plan(int32_t weight_type, uint32_t flags, int32_t rows, int32_t ntok, int32_t out[7]) {
    if (!out || rows < 1 || ntok < 1) return GL3_E_ARG;
    if (weight_type != GL3_TYPE_F16 && weight_type != GL3_TYPE_Q4_0 && weight_type != GL3_TYPE_Q8_0) return GL3_E_ARG;
    // the plans that batch on these GEMMs: Vector-API order; Q8_0 only with the f32 activation, 512 bits only for F16 (gl3_create)
    if ((flags & GL3_FLAG_SCALAR_DOT) || (flags & GL3_FLAG_VECTOR_128) || ((flags & GL3_FLAG_F32_ACTIVATION) != 0) != (weight_type == GL3_TYPE_Q8_0) ||
        ((flags & GL3_FLAG_VECTOR_512) && weight_type != GL3_TYPE_F16))
        return GL3_E_ARG;
    const VlGemmPlan p = vl_gemm_plan(weight_type == GL3_TYPE_Q8_0 ? GL3_FMT_Q8V : weight_type, (flags & GL3_FLAG_VECTOR_512) != 0, rows, ntok, vl_gemm_switches());
    out[0] = p.kernel; out[1] = p.nrt; out[2] = p.ntt; out[3] = p.grid; out[4] = p.xcd_tokens; out[5] = p.G; out[6] = p.P;
    return GL3_OK;
}

// The same layers for F16 / Q4_0 / Q8_0-with-f32-activation matrices: RMSNorm to f32 (exact sum of squares), GEMMs on the f32
// activations, gate and up as two GEMMs + an element-wise SwiGLU.  Tensor parallel (r4): the row-split matrices write this rank's
// chunk of the rank-chunked X / AO / HB (as the int8 path does), the gathers are in place, and the next GEMM's operand is the
// gathered activation un-chunked (or normalised) into XN.
static int32_t pf_layers_vl(gl3_ctx* ctx, const PfStep& st) {
    const int n = st.n;
    Gl3Range chunk_range("gl3 batched step, tokens", n);
    gl3_prefill_state* p = ctx->pf;
    const gl3_model_desc& d = ctx->d;
    hipStream_t s = ctx->stream;
    const int rank = d.tp_rank, tp = d.tp_size, qd = ctx->q_dim_l, kvd = ctx->kv_dim_l, hid = ctx->hidden_l, dml = ctx->dim_l;
    const int qkv_dim = qd + 2 * kvd;
    float* Xr = p->X + (size_t)rank * n * dml;
    float* AOr = p->AO + (size_t)rank * n * qd;
    float* HBr = p->HB + (size_t)rank * n * hid;
    int32_t r;
    // every rank holds the whole embedding table: the full X, written in the rank-chunked layout
    if (ctx->emb.fmt == GL3_TYPE_F16) hipLaunchKernelGGL((pf_embed_vl_kernel<WT_F16>), dim3(n), dim3(256), 0, s, ctx->emb.w, d.dim, p->tokens, p->X, ctx->emb_scale, dml);
    else if (ctx->emb.fmt == GL3_TYPE_Q4_0) hipLaunchKernelGGL((pf_embed_vl_kernel<WT_Q4_0>), dim3(n), dim3(256), 0, s, ctx->emb.w, d.dim, p->tokens, p->X, ctx->emb_scale, dml);
    else hipLaunchKernelGGL((pf_embed_vl_kernel<WT_Q8_0>), dim3(n), dim3(256), 0, s, ctx->emb.w, d.dim, p->tokens, p->X, ctx->emb_scale, dml);
    const PfOperand xn = pf_operand_f32(p);
    for (int l = 0; l < d.n_layers; ++l) {
        gl3_layer& L = ctx->layers[l];
        Gl3Range layer_range("layer", l);
        pf_quant<PQ_NORM_F32>(ctx, p->X, d.dim, dml, L.attn_norm, n, xn);
        launch_gemm_vl<EPI_STORE>(ctx, L.wqkv, n, p->XN, d.dim, p->QKV, qkv_dim);
        pf_attention(ctx, l, st, AOr, false);
        if ((r = gl3_all_gather(ctx, GB_PF_AO, (size_t)n * qd)) != GL3_OK) return r;
        const float* ao = p->AO;
        if (tp > 1) { pf_quant<PQ_PLAIN_F32>(ctx, p->AO, ctx->q_dim, qd, nullptr, n, xn); ao = p->XN; }      // rank-chunked [tp][n][qd] -> plain XN[n][q_dim]
        if (ctx->wo_replicated) {
            // every rank holds all of Wo: one GEMM per rank chunk of the rank-chunked X (rows [c dml, (c + 1) dml) -> chunk c), no gather
            for (int c = 0; c < tp; ++c) {
                Q8Mat sub = L.wo;
                sub.rows = dml;
                sub.w = L.wo.w + (size_t)(c * dml / 8) * L.wo.vl_group_bytes();
                launch_gemm_vl<EPI_RESID>(ctx, sub, n, ao, ctx->q_dim, p->X + (size_t)c * n * dml, dml, ctx->resid_scale);
            }
        } else {
            launch_gemm_vl<EPI_RESID>(ctx, L.wo, n, ao, ctx->q_dim, Xr, dml, ctx->resid_scale);
            if ((r = gl3_all_gather(ctx, GB_PF_X, (size_t)n * dml)) != GL3_OK) return r;
        }
        pf_quant<PQ_NORM_F32>(ctx, p->X, d.dim, dml, L.ffn_norm, n, xn);
        launch_gemm_vl<EPI_STORE>(ctx, L.w1, n, p->XN, d.dim, HBr, hid);
        launch_gemm_vl<EPI_STORE>(ctx, L.w3, n, p->XN, d.dim, p->HB2, hid);
        const size_t ne = (size_t)n * hid;
        hipLaunchKernelGGL(pf_swiglu_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, HBr, p->HB2, ne);
        if ((r = gl3_all_gather(ctx, GB_PF_HB, (size_t)n * hid)) != GL3_OK) return r;
        const float* hb = p->HB;
        if (tp > 1) { pf_quant<PQ_PLAIN_F32>(ctx, p->HB, d.hidden, hid, nullptr, n, xn); hb = p->XN; }
        launch_gemm_vl<EPI_RESID>(ctx, L.w2, n, hb, d.hidden, Xr, dml, ctx->resid_scale);
        if ((r = gl3_all_gather(ctx, GB_PF_X, (size_t)n * dml)) != GL3_OK) return r;
    }
    GL3_HIP(hipGetLastError());
    return GL3_OK;
}

// The Qwen2-MoE feed-forward block of layer l for the n tokens of a step (one rank) — InferenceCore.forwardJavaQwen2MoE :363-415 per
// token: xb = rmsnorm(x) quantised ONCE is the operand of the router's f32 rows (which normalise x themselves, as in the decode
// step), of every selected expert and of the shared expert.  Router -> grouping by expert -> routed gate + up / down as grouped GEMMs
// over the tile table -> shared expert on the dense GEMMs, its down projection stored into y[token][topk] -> combine.
static void pf_moe_ffn(gl3_ctx* ctx, int l, int n) {
    gl3_prefill_state* p = ctx->pf;
    auto& m = p->moe;
    const gl3_model_desc& d = ctx->d;
    hipStream_t s = ctx->stream;
    gl3_layer& L = ctx->layers[l];
    const int E = d.n_experts, topk = d.n_experts_used, mh = d.moe_hidden, S = n * topk;
    {   Gl3Range g("moe: rmsnorm + router + top-k");
        MoeRouterArgs ra{};
        ra.x = p->X; ra.norm_w = L.ffn_norm; ra.eps = d.rms_eps; ra.gate_inp = L.gate_inp; ra.gate_inp_shexp = L.gate_inp_shexp;
        ra.dim = d.dim; ra.n_experts = E; ra.topk = topk; ra.logits = m.logits; ra.w_out = m.w; ra.sel = m.sel; ra.ticket = m.ticket;
        hipLaunchKernelGGL(moe_router_batch_kernel, dim3(moe_router_wgs(E), n), dim3(256), moe_router_smem(d.dim, E), s, ra);
        hipLaunchKernelGGL(moe_group_kernel, dim3(1), dim3(MOE_GROUP_THREADS), moe_group_smem(E), s, m.sel, n, topk, E, m.slot_tok, m.slot_dst, m.tab); }
    PfOperand xb = pf_operand(p, n);
    pf_quant<PQ_NORM>(ctx, p->X, d.dim, d.dim, L.ffn_norm, n, xb);
    if (pf_chunk_major(n)) {      // the chunk-major operand serves the shared expert; the routed experts read the XQ2 / XS2 layout
        xb = {m.XQx, m.XSx, p->maxk, m.ts_x, nullptr, 0};
        pf_quant<PQ_NORM>(ctx, p->X, d.dim, d.dim, L.ffn_norm, n, xb);
    }
    {   Gl3Range g("moe: routed experts");
        launch_gemm_grouped<EPI_SWIGLU>(ctx, L.gate_exps, &L.up_exps, mh, n, xb.XQ, xb.XS, xb.tslots, m.slot_tok, nullptr, m.HB, mh);
        // hb per 32-block as matmulExpert quantises it (Q8_0FloatTensor.java:96-118); row = sorted slot, so a token tile is 16 consecutive rows
        pf_quant<PQ_PLAIN>(ctx, m.HB, mh, mh, nullptr, S, {m.XQh, m.XSh, mh, m.ts_h, nullptr, 0});
        launch_gemm_grouped<EPI_STORE>(ctx, L.down_exps, nullptr, d.dim, n, m.XQh, m.XSh, m.ts_h, nullptr, m.slot_dst, m.Y, d.dim); }
    {   Gl3Range g("moe: shared expert");      // after the routed gate + up: the unfused hand-over below overwrites xb
        float* ysh = m.Y + (size_t)topk * d.dim;
        const int ystride = (topk + 1) * d.dim;
        const bool fuse_off = pf_fused_quant_off();
        const bool fuse_q = !fuse_off && bd_tslots(n) != 0 && (d.hidden % 32) == 0;
        const bool fuse_big = !fuse_off && pf_chunk_major(n) && p->XQh && gl3_gemm3_swiglu_quantises(L.w1.rows, n);
        if (fuse_q || fuse_big) {
            launch_gemm<EPI_SWIGLU>(ctx, L.w1, &L.w3, n, p->HB, d.hidden, 1.0f, false, true);
            launch_gemm<EPI_STORE>(ctx, L.w2, nullptr, n, ysh, ystride, 1.0f, true);
        } else {
            launch_gemm<EPI_SWIGLU>(ctx, L.w1, &L.w3, n, p->HB, d.hidden);
            pf_quant<PQ_PLAIN>(ctx, p->HB, d.hidden, d.hidden, nullptr, n, pf_operand(p, n));
            launch_gemm<EPI_STORE>(ctx, L.w2, nullptr, n, ysh, ystride);
        } }
    {   Gl3Range g("moe: weighted accumulation into x");
        hipLaunchKernelGGL(moe_combine_kernel, dim3((d.dim + 255) / 256, n), dim3(256), 0, s, p->X, m.Y, m.w, d.dim, topk + 1); }
}

// Parity taps gl3_get_buffer 9 / 10: the routing of the last layer of the last batched step, rows in step order — weights
// [rows][topk + 1] (9), expert ids as floats [rows][topk] (10).
int32_t gl3_prefill_moe_tap(gl3_ctx* ctx, int which, float* out, uint64_t n) {
    gl3_prefill_state* p = ctx->pf;
    if (!p || !p->moe.w) GL3_FAIL(GL3_E_STATE, "not a qwen2moe plan with batched buffers (max_batch > 1)");
    const uint64_t per = which == 9 ? ctx->d.n_experts_used + 1 : ctx->d.n_experts_used;
    if (n > (uint64_t)p->max_batch * per) GL3_FAIL(GL3_E_ARG, "buffer shorter than requested");
    GL3_HIP(hipSetDevice(ctx->d.device));
    GL3_HIP(hipStreamSynchronize(ctx->stream));
    if (which == 9) { GL3_HIP(hipMemcpy(out, p->moe.w, n * sizeof(float), hipMemcpyDeviceToHost)); return GL3_OK; }
    std::vector<int> ids(n);
    GL3_HIP(hipMemcpy(ids.data(), p->moe.sel, n * sizeof(int), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; ++i) out[i] = (float)ids[i];
    return GL3_OK;
}

// All layers for the st.n tokens of a step whose (token, sequence, position) — and, for st.ntab > 0, tile table — are already on the device.
static int32_t pf_layers(gl3_ctx* ctx, const PfStep& st) {
    const int n = st.n;
    Gl3Range chunk_range("gl3 batched step, tokens", n);
    gl3_prefill_state* p = ctx->pf;
    if (p->vl) return pf_layers_vl(ctx, st);
    const gl3_model_desc& d = ctx->d;
    hipStream_t s = ctx->stream;
    // tensor parallel: this rank's heads / hidden units / dim rows; activations that are gathered use the rank-chunked layout
    const int rank = d.tp_rank, qd = ctx->q_dim_l, kvd = ctx->kv_dim_l;
    const int hid = ctx->hidden_l, dml = ctx->dim_l;
    const int qkv_dim = qd + 2 * kvd;
    const bool fused_decode = pf_fused_decode(ctx, st);
    // small batch on one rank: the attention output and hb leave their kernels already quantised for the next GEMM (no
    // separate quantise launches; under tensor parallelism the f32 vectors are gathered first, so the launches stay)
    const bool fuse_off = pf_fused_quant_off();
    const bool fuse_q = !fuse_off && bd_tslots(n) != 0 && d.tp_size == 1 && (d.hidden % 32) == 0 && (d.head_size % 32) == 0;
    float* Xr = p->X + (size_t)rank * n * dml;           // this rank's chunk of X / AO / HB
    float* AOr = p->AO + (size_t)rank * n * qd;
    float* HBr = p->HB + (size_t)rank * n * hid;
    const PfOperand xq = pf_operand(p, n);
    int32_t r;
    hipLaunchKernelGGL(pf_embed_kernel, dim3(n), dim3(256), 0, s, ctx->emb.w, ctx->emb.ng, d.dim, p->tokens, p->X, dml, ctx->emb_scale);
    for (int l = 0; l < d.n_layers; ++l) {
        gl3_layer& L = ctx->layers[l];
        Gl3Range layer_range("layer", l);
        pf_quant<PQ_NORM>(ctx, p->X, d.dim, dml, L.attn_norm, n, xq);
        launch_gemm<EPI_STORE>(ctx, L.wqkv, nullptr, n, p->QKV, qkv_dim);
        const bool quantised_ao = pf_attention(ctx, l, st, AOr, fuse_q && st.one_seq < 0 && fused_decode);
        if ((r = gl3_all_gather(ctx, GB_PF_AO, (size_t)n * qd)) != GL3_OK) return r;
        if (!quantised_ao) pf_quant<PQ_PLAIN>(ctx, p->AO, ctx->q_dim, qd, nullptr, n, xq);
        if (ctx->wo_replicated) {
            // every rank holds all of Wo: one GEMM per rank chunk of the rank-chunked X (rows [c dml, (c + 1) dml) -> chunk c), no gather
            for (int c = 0; c < d.tp_size; ++c) {
                Q8Mat sub = L.wo;
                sub.rows = dml; sub.nstrips = (dml + 15) / 16;
                sub.w = L.wo.w + (size_t)(c * dml / 16) * L.wo.ng * TILE_BYTES;
                launch_gemm<EPI_RESID>(ctx, sub, nullptr, n, p->X + (size_t)c * n * dml, dml, ctx->resid_scale);
            }
        } else {
            launch_gemm<EPI_RESID>(ctx, L.wo, nullptr, n, Xr, dml, ctx->resid_scale);
            if ((r = gl3_all_gather(ctx, GB_PF_X, (size_t)n * dml)) != GL3_OK) return r;
        }
        if (d.arch == GL3_ARCH_QWEN2MOE) { pf_moe_ffn(ctx, l, n); continue; }
        pf_quant<PQ_NORM>(ctx, p->X, d.dim, dml, L.ffn_norm, n, xq);
        // > 64 tokens on one rank: the tall gate + up tiling writes hb quantised (no f32 round trip, no quantise launch)
        const bool fuse_big = !fuse_off && pf_chunk_major(n) && d.tp_size == 1 && p->XQh && gl3_gemm3_swiglu_quantises(L.w1.rows, n);
        if (fuse_q || fuse_big) {
            launch_gemm<EPI_SWIGLU>(ctx, L.w1, &L.w3, n, HBr, hid, 1.0f, false, true);
            launch_gemm<EPI_RESID>(ctx, L.w2, nullptr, n, Xr, dml, ctx->resid_scale, true);
        } else {
            launch_gemm<EPI_SWIGLU>(ctx, L.w1, &L.w3, n, HBr, hid);
            if ((r = gl3_all_gather(ctx, GB_PF_HB, (size_t)n * hid)) != GL3_OK) return r;
            pf_quant<PQ_PLAIN>(ctx, p->HB, d.hidden, hid, nullptr, n, xq);
            launch_gemm<EPI_RESID>(ctx, L.w2, nullptr, n, Xr, dml, ctx->resid_scale);
        }
        if ((r = gl3_all_gather(ctx, GB_PF_X, (size_t)n * dml)) != GL3_OK) return r;
    }
    GL3_HIP(hipGetLastError());
    return GL3_OK;
}

int32_t gl3_prefill_attn_rows(gl3_ctx* ctx, int32_t out[4]) {
    gl3_prefill_state* p = ctx->pf;
    if (!p || !p->attn_rows_set) GL3_FAIL(GL3_E_STATE, "gl3_get_attn_rows before any batched step");
    for (int i = 0; i < 4; ++i) out[i] = p->attn_rows[i];
    return GL3_OK;
}

float* gl3_prefill_buf(gl3_ctx* ctx, int which) {
    gl3_prefill_state* p = ctx->pf;
    return which == GB_PF_X ? p->X : which == GB_PF_AO ? p->AO : which == GB_PF_HB ? p->HB : p->LOGITS;
}

// x of token b from the rank-chunked X into the decode path's plain ctx->x (parity tap gl3_get_x)
static __global__ void pf_unchunk_row_kernel(const float* __restrict__ X, int b, int dim, int cc, int ntok, float* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < dim; i += gridDim.x * blockDim.x) out[i] = X[chunked(b, i, cc, ntok)];
}

static int32_t pf_stage_tokens(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seqs, const int32_t* poss, int n) {
    gl3_prefill_state* p = ctx->pf;
    GL3_HIP(hipMemcpyAsync(p->tokens, tokens, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    GL3_HIP(hipMemcpyAsync(p->seqpos, seqs, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    GL3_HIP(hipMemcpyAsync(p->seqpos + p->max_batch, poss, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    return GL3_OK;
}

int32_t gl3_prefill_run(gl3_ctx* ctx, int32_t seq, const int32_t* tokens, int32_t n, int32_t start_pos) {
    gl3_prefill_state* p = ctx->pf;
    const gl3_model_desc& d = ctx->d;
    for (int i = 0; i < n; ++i)
        if (tokens[i] < 0 || tokens[i] >= d.vocab) GL3_FAIL(GL3_E_ARG, "token id out of range");
    GL3_HIP(hipSetDevice(d.device));
    std::vector<int32_t> seqs(n, seq), poss(n);
    for (int i = 0; i < n; ++i) poss[i] = start_pos + i;
    int32_t r = pf_stage_tokens(ctx, tokens, seqs.data(), poss.data(), n);
    if (r != GL3_OK) return r;
    if ((r = pf_layers(ctx, PfStep{n, start_pos + n - 1, seq, 0})) != GL3_OK) return r;
    // keep the decode path's x in step with the last prefilled token (parity tap gl3_get_x)
    hipLaunchKernelGGL(pf_unchunk_row_kernel, dim3(4), dim3(256), 0, ctx->stream, p->X, n - 1, d.dim, ctx->dim_l, n, ctx->x);
    GL3_HIP(hipStreamSynchronize(ctx->stream));
    return gl3_tp_check(ctx);
}

// The logits stage of a step: output RMSNorm + vocabulary projection of `rows` rows of src (rank-chunked, chunk width src_cc) -> rows of
// dst_stride floats at dst_chunk.  Vocabulary rows are split across ranks: dst_chunk is this rank's chunk of the rank-chunked logits.
static void pf_logits_stage(gl3_ctx* ctx, const float* src, int src_cc, int rows, float* dst_chunk, int dst_stride) {
    gl3_prefill_state* p = ctx->pf;
    const int dim = ctx->d.dim;
    if (p->vl) {
        pf_quant<PQ_NORM_F32>(ctx, src, dim, src_cc, ctx->out_norm, rows, pf_operand_f32(p));
        launch_gemm_vl<EPI_STORE>(ctx, ctx->wcls, rows, p->XN, dim, dst_chunk, dst_stride, ctx->logit_scale);
    } else {
        pf_quant<PQ_NORM>(ctx, src, dim, src_cc, ctx->out_norm, rows, pf_operand(p, rows));
        launch_gemm<EPI_STORE>(ctx, ctx->wcls, nullptr, rows, dst_chunk, dst_stride, ctx->logit_scale);
    }
}

// Greedy ids of the first `rows` rows of p->LOGITS (rank-chunked, chunk width cc) -> p->amax
static void pf_greedy(gl3_ctx* ctx, int rows, int cc) {
    gl3_prefill_state* p = ctx->pf;
    hipLaunchKernelGGL(pf_argmax_part_kernel, dim3(AMX_SPLIT, rows), dim3(256), 0, ctx->stream, p->LOGITS, ctx->d.vocab, cc, p->amx_v, p->amx_i);
    hipLaunchKernelGGL(pf_argmax_fold_kernel, dim3(rows), dim3(64), 0, ctx->stream, p->amx_v, p->amx_i, p->amax);
}

// One decode step of n independent sequences = the prefill machinery over (token, sequence, position) triples +
// final RMSNorm + vocab projection for every row (the n matvecs become one GEMM over the shared weights).
static int32_t pf_grow_logits(gl3_ctx* ctx, int n) {
    gl3_prefill_state* p = ctx->pf;
    const gl3_model_desc& d = ctx->d;
    if (p->logits_rows < n && p->in_arena) GL3_FAIL(GL3_E_UNSUPPORTED, "tensor-parallel static-batched decode is limited to 64 sequences per step");
    if (p->logits_rows < n) {
        for (auto& ge : p->step_graphs) if (ge) { hipGraphExecDestroy(ge); ge = nullptr; }      // captured steps point at the old buffer
        if (p->LOGITS) hipFree(p->LOGITS);
        p->LOGITS = nullptr; p->logits_rows = 0;
        GL3_HIP(hipMalloc((void**)&p->LOGITS, (size_t)n * d.vocab * 4));
        p->logits_rows = n;
    }
    return GL3_OK;
}

// The batched sampler's view of a step (gl3_sample.hip): the logits rows and the greedy ids, both on the device.
void gl3_decode_batch_outputs(gl3_ctx* ctx, const float** logits, const int32_t** greedy) {
    *logits = ctx->pf->LOGITS; *greedy = ctx->pf->amax;
}

// The logits tail of a batched step, shared by the static-batched and the mixed step: output RMSNorm + vocabulary projection of `rows` rows
// of src (rank-chunked, chunk width src_cc) into this rank's chunk [rows][vocab / tp] of the rank-chunked p->LOGITS, the gather, and the
// greedy ids of the gathered rows.  One rank: the chunk is the plain [rows][vocab] buffer and nothing is gathered.
static int32_t pf_logits_tail(gl3_ctx* ctx, const float* src, int src_cc, int rows) {
    gl3_prefill_state* p = ctx->pf;
    const int vl = ctx->vocab_l;
    pf_logits_stage(ctx, src, src_cc, rows, p->LOGITS + (size_t)ctx->d.tp_rank * rows * vl, vl);
    const int32_t r = gl3_all_gather(ctx, GB_PF_LOGITS, (size_t)rows * vl);
    if (r != GL3_OK) return r;
    pf_greedy(ctx, rows, vl);
    return GL3_OK;
}

// The first `rows` rows of p->LOGITS <-> plain host rows [rows][vocab]: one copy on one rank, one 2D copy per rank chunk of the
// rank-chunked [tp][rows][vocab / tp] buffer otherwise
static int32_t pf_logits_copy(gl3_ctx* ctx, float* host, int rows, hipMemcpyKind kind) {
    gl3_prefill_state* p = ctx->pf;
    const gl3_model_desc& d = ctx->d;
    const int vl = ctx->vocab_l;
    const bool out = kind == hipMemcpyDeviceToHost;
    if (d.tp_size == 1) {
        GL3_HIP(hipMemcpyAsync(out ? (void*)host : (void*)p->LOGITS, out ? (const void*)p->LOGITS : (const void*)host, (size_t)rows * d.vocab * 4, kind, ctx->stream));
        return GL3_OK;
    }
    for (int c = 0; c < d.tp_size; ++c) {
        float* dev = p->LOGITS + (size_t)c * rows * vl;
        float* hst = host + (size_t)c * vl;
        if (out) GL3_HIP(hipMemcpy2DAsync(hst, (size_t)d.vocab * 4, dev, (size_t)vl * 4, (size_t)vl * 4, rows, kind, ctx->stream));
        else GL3_HIP(hipMemcpy2DAsync(dev, (size_t)vl * 4, hst, (size_t)d.vocab * 4, (size_t)vl * 4, rows, kind, ctx->stream));
    }
    return GL3_OK;
}

// Parity taps gl3_sample_rows / gl3_score_rows / gl3_verify_rows: caller-supplied plain [n][vocab] logits take the place of a step's — laid
// out as a step leaves them, rank-chunked under tensor parallelism, so the taps exercise the chunked readers — followed by the step's own
// greedy scan.  No forward pass, no KV change, no peer; nothing is waited for.
int32_t gl3_decode_batch_load_logits(gl3_ctx* ctx, const float* logits, int32_t n) {
    const gl3_model_desc& d = ctx->d;
    GL3_HIP(hipSetDevice(d.device));
    int32_t r = pf_grow_logits(ctx, n);
    if (r != GL3_OK) return r;
    if ((r = pf_logits_copy(ctx, const_cast<float*>(logits), n, hipMemcpyHostToDevice)) != GL3_OK) return r;
    pf_greedy(ctx, n, ctx->vocab_l);
    GL3_HIP(hipGetLastError());
    return GL3_OK;
}

// The static-batched step in two halves, so that a chain of steps (gl3_forward_decode_batch_chain) stages once and enqueues k times:
// stage = room for n logits rows and the n (token, sequence, position) triples up; enqueue = one step of n rows whose deepest row is at
// max_pos, the only thing the host takes from the positions.  The rows' own positions are read from p->seqpos by every attention form such
// a step can take (attn_head_kernel: posv; pf_rope_kv_kernel and the per-row pair behind it: RopeArgs / PfAttnArgs::pos).
int32_t gl3_decode_batch_stage(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions, int32_t n) {
    GL3_HIP(hipSetDevice(ctx->d.device));
    const int32_t r = pf_grow_logits(ctx, n);
    return r != GL3_OK ? r : pf_stage_tokens(ctx, tokens, seq_ids, positions, n);
}

// The step's inputs on the device: what a chained step's hand-over launch rewrites for the step behind it (gl3_sample.hip)
void gl3_decode_batch_inputs(gl3_ctx* ctx, int32_t** tokens, int32_t** positions) {
    *tokens = ctx->pf->tokens; *positions = ctx->pf->seqpos + ctx->pf->max_batch;
}

int32_t gl3_decode_batch_enqueue(gl3_ctx* ctx, int32_t n, int32_t max_pos) {
    gl3_prefill_state* p = ctx->pf;
    const gl3_model_desc& d = ctx->d;
    int32_t r;
    hipStream_t s = ctx->stream;
    // the whole step: layers, final RMSNorm + vocabulary projection of every row, greedy ids
    auto enqueue_step = [&](const PfStep& st) -> int32_t {
        const int32_t rr = pf_layers(ctx, st);
        return rr != GL3_OK ? rr : pf_logits_tail(ctx, p->X, ctx->dim_l, n);
    };
    // ~400 launches per step: replay them as one hipGraph per batch size.  Nothing position-dependent is baked in when every
    // position is below AF_MAXN (the one-launch attention reads sequence ids / positions from device memory).  The three-kernel
    // attention (GL3_NO_FUSED_BD_ATTN=1) sizes its scores grid by the deepest row: a step captured at position 0 would score the
    // first 64 positions only, so those steps stay eager.
    static const bool graphs_off = env_flag("GL3_NO_GRAPH", false);
    const PfStep st{n, max_pos, -1, 0};
    const bool graphable = !graphs_off && !gl3_roctx_on() && !(d.flags & GL3_FLAG_NO_GRAPH) && pf_fused_decode(ctx, st) && ctx->transport != GL3_TP_RCCL;
    if (graphable) {
        if ((int)p->step_graphs.size() <= n) p->step_graphs.resize(n + 1, nullptr);
        if (!p->step_graphs[n]) {
            hipGraph_t g = nullptr;
            GL3_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            r = enqueue_step(PfStep{n, 0, -1, 0});      // any depth below AF_MAXN enqueues the same launches: the capture names position 0
            const hipError_t e = hipStreamEndCapture(s, &g);
            if (r != GL3_OK) return r;
            GL3_HIP(e);
            GL3_HIP(hipGraphInstantiate(&p->step_graphs[n], g, nullptr, nullptr, 0));
            hipGraphDestroy(g);
        }
        GL3_HIP(hipGraphLaunch(p->step_graphs[n], s));
        p->attn_rows[0] = n; p->attn_rows[1] = p->attn_rows[2] = p->attn_rows[3] = 0; p->attn_rows_set = true;      // a replay does not pass pf_attention: the captured step is attn_head_kernel's
    } else if ((r = enqueue_step(st)) != GL3_OK) return r;
    GL3_HIP(hipGetLastError());
    return GL3_OK;
}

int32_t gl3_decode_batch_run(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions, int32_t n,
                             float* logits_out, int32_t* argmax_out, bool finish) {
    gl3_prefill_state* p = ctx->pf;
    int32_t r = gl3_decode_batch_stage(ctx, tokens, seq_ids, positions, n);
    if (r != GL3_OK) return r;
    int max_pos = 0;
    for (int i = 0; i < n; ++i) max_pos = positions[i] > max_pos ? positions[i] : max_pos;
    if ((r = gl3_decode_batch_enqueue(ctx, n, max_pos)) != GL3_OK) return r;
    hipStream_t s = ctx->stream;
    if (argmax_out) GL3_HIP(hipMemcpyAsync(argmax_out, p->amax, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (logits_out && (r = pf_logits_copy(ctx, logits_out, n, hipMemcpyDeviceToHost)) != GL3_OK) return r;      // un-chunked on the way out
    GL3_HIP(hipGetLastError());
    if (!finish) return GL3_OK;          // the batched sampler's launches follow on the same stream (gl3_sample_batch_finish)
    GL3_HIP(hipStreamSynchronize(s));
    return gl3_tp_check(ctx);
}

// ---------------------------------------------------------------------------------------------------
// Mixed step (gl3_forward_batch): prompt chunks and decode rows of many sequences in one pass over the weights.  The layers are pf_layers
// over (token, sequence, position) rows as in a static-batched step; the attention takes the run-table form (pf_attention); the logits stage
// runs over the rows the caller flagged only.  Eager: the shape of a step differs from call to call.
// Tensor parallel: the layers and the run-table attention forms work on this rank's heads and chunks as in every other batched step (the
// table records name step rows, sequences and positions, nothing per head); the flagged rows are gathered out of the rank-chunked X into
// plain rows, and the logits tail is the static-batched step's (pf_logits_tail): this rank's vocabulary chunk, the gather into the arena's
// rank-chunked logits — which hold min(max_batch, 64) rows: a step with more output rows is refused with the arguments (gl3_api.hip) —
// and the greedy scan.  Every rank then holds every output row, and the sampler / scorer behind the step read them redundantly.
static_assert(BP_TILE_ROWS == FA_TB, "the step plan cuts runs into the attention kernels' token tiles");
static_assert(BP_DEEP_ROWS == PA_TB && BP_DEEP_ROWS == SCM_TB && BP_DEEP_ROWS == PVM_TB && BP_DEEP_ROWS <= PVR_TB,
              "the step plan cuts deep rows into the long-context kernels' token tiles (one record per workgroup of pf_pv_ring_kernel)");
static_assert(sizeof(BatchSpan) == sizeof(int4), "a tile record is read as one int4");

// rows[r] of the ntok rows of X (rank-chunked, chunk width cc; cc = dim: plain rows) -> row r of out, plain (float4 per thread; cc % 4 == 0)
static __global__ __launch_bounds__(256) void pf_gather_rows_kernel(const float* __restrict__ X, const int32_t* __restrict__ rows, int dim, int cc, int ntok,
                                                                    float* __restrict__ out) {
    const int b = rows[blockIdx.x];
    float4* dst = reinterpret_cast<float4*>(out + (size_t)blockIdx.x * dim);
    for (int i = threadIdx.x; i < (dim >> 2); i += 256) dst[i] = *reinterpret_cast<const float4*>(X + chunked(b, 4 * i, cc, ntok));
}

// x of row `row` of the n-row step the stream just ran -> the decode path's ctx->x (parity tap gl3_get_x), waited for
int32_t gl3_prefill_tap_x(gl3_ctx* ctx, int row, int n) {
    hipLaunchKernelGGL(pf_unchunk_row_kernel, dim3(4), dim3(256), 0, ctx->stream, ctx->pf->X, row, ctx->d.dim, ctx->dim_l, n, ctx->x);
    GL3_HIP(hipStreamSynchronize(ctx->stream));
    return GL3_OK;
}

int32_t gl3_batch_run(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions, int32_t n, const BatchPlan& bp,
                      float* logits_out, int32_t* argmax_out, bool finish) {
    gl3_prefill_state* p = ctx->pf;
    const gl3_model_desc& d = ctx->d;
    const int n_out = (int)bp.out_rows.size();
    GL3_HIP(hipSetDevice(d.device));
    if (n_out) {
        const int32_t r0 = pf_grow_logits(ctx, n_out);
        if (r0 != GL3_OK) return r0;
        if (!p->XG) GL3_HIP(hipMalloc((void**)&p->XG, (size_t)p->max_batch * d.dim * 4));
    }
    hipStream_t s = ctx->stream;
    int32_t r = pf_stage_tokens(ctx, tokens, seq_ids, positions, n);
    if (r != GL3_OK) return r;
    // a step with a run of several rows: its tiles by depth (shallow: the one-launch table form; deep: the long-context trio), staged with the tokens
    BatchSplit sp;
    if (!bp.single_rows) batch_plan_split(bp, p->tab_max_pos, sp);
    const int ntab = (int)sp.shallow.size(), ndeep = (int)sp.deep.size(), deep_rows = (int)sp.deep_rows.size();
    if (ntab) GL3_HIP(hipMemcpyAsync(p->tiles, sp.shallow.data(), (size_t)ntab * sizeof(BatchSpan), hipMemcpyHostToDevice, s));
    if (ndeep) {
        GL3_HIP(hipMemcpyAsync(p->deep, sp.deep.data(), (size_t)ndeep * sizeof(BatchSpan), hipMemcpyHostToDevice, s));
        GL3_HIP(hipMemcpyAsync(p->deep_rows, sp.deep_rows.data(), (size_t)deep_rows * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    if (n_out) GL3_HIP(hipMemcpyAsync(p->out_rows, bp.out_rows.data(), (size_t)n_out * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if ((r = pf_layers(ctx, PfStep{n, bp.max_pos, -1, ntab, ndeep, deep_rows, sp.shallow_max_pos})) != GL3_OK) return r;
    // keep the decode path's x in step with the last row (parity tap gl3_get_x)
    hipLaunchKernelGGL(pf_unchunk_row_kernel, dim3(4), dim3(256), 0, s, p->X, n - 1, d.dim, ctx->dim_l, n, ctx->x);
    if (n_out) {      // output RMSNorm + vocabulary projection + greedy ids of the flagged rows, compact
        hipLaunchKernelGGL(pf_gather_rows_kernel, dim3(n_out), dim3(256), 0, s, p->X, p->out_rows, d.dim, ctx->dim_l, n, p->XG);
        if ((r = pf_logits_tail(ctx, p->XG, d.dim, n_out)) != GL3_OK) return r;
        if (argmax_out) GL3_HIP(hipMemcpyAsync(argmax_out, p->amax, (size_t)n_out * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (logits_out && (r = pf_logits_copy(ctx, logits_out, n_out, hipMemcpyDeviceToHost)) != GL3_OK) return r;      // un-chunked on the way out
    }
    GL3_HIP(hipGetLastError());
    if (!finish) return GL3_OK;          // the batched sampler's launches follow on the same stream (gl3_sample_batch_finish)
    GL3_HIP(hipStreamSynchronize(s));
    return gl3_tp_check(ctx);
}


// Average device time of one batched-prefill GEMM class at n tokens: one HIP event pair around `iters` sweeps over every
// layer's weights (GEMMs are 70-250 us, the ~1.5 us boundary is noise).  int8_ops = 2 * rows * K * n per launch (MFMA work
// only; the f32 scale-and-accumulate epilogue the reference arithmetic needs is not counted).
int32_t gl3_prefill_profile(gl3_ctx* ctx, int klass, int n, int iters, double* out_us, uint64_t* int8_ops) {
    gl3_prefill_state* p = ctx->pf;
    const gl3_model_desc& d = ctx->d;
    if (!p || p->vl) GL3_FAIL(GL3_E_UNSUPPORTED, "the int8 GEMM profile needs max_batch > 1 and Q8_0 weights with the int8 activation");
    if (n < 1 || n > p->max_batch) GL3_FAIL(GL3_E_ARG, "token count outside 1..max_batch");
    GL3_HIP(hipSetDevice(d.device));
    const int qkv_dim = ctx->q_dim_l + 2 * ctx->kv_dim_l;
    auto sweep = [&]() {
        for (int l = 0; l < d.n_layers; ++l) {
            gl3_layer& L = ctx->layers[l];
            switch (klass) {
            case GL3_K_MATVEC_QKV: launch_gemm<EPI_STORE>(ctx, L.wqkv, nullptr, n, p->QKV, qkv_dim); break;
            case GL3_K_MATVEC_WO: launch_gemm<EPI_RESID>(ctx, L.wo, nullptr, n, p->X, ctx->wo_rows); break;
            case GL3_K_MATVEC_GATEUP: launch_gemm<EPI_SWIGLU>(ctx, L.w1, &L.w3, n, p->HB, ctx->hidden_l); break;
            default: launch_gemm<EPI_RESID>(ctx, L.w2, nullptr, n, p->X, ctx->dim_l); break;
            }
        }
    };
    hipEvent_t e0, e1;
    GL3_HIP(hipEventCreate(&e0)); GL3_HIP(hipEventCreate(&e1));
    sweep();
    GL3_HIP(hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < iters; ++i) sweep();
    GL3_HIP(hipEventRecord(e1, ctx->stream));
    GL3_HIP(hipEventSynchronize(e1));
    float ms = 0;
    GL3_HIP(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    *out_us = (double)ms * 1e3 / ((double)iters * d.n_layers);
    if (int8_ops) {
        const gl3_layer& L = ctx->layers[0];
        const Q8Mat& w = klass == GL3_K_MATVEC_QKV ? L.wqkv : klass == GL3_K_MATVEC_WO ? L.wo : klass == GL3_K_MATVEC_GATEUP ? L.w1 : L.w2;
        *int8_ops = (uint64_t)2 * w.rows * w.k * n * (klass == GL3_K_MATVEC_GATEUP ? 2 : 1);
    }
    return GL3_OK;
}
