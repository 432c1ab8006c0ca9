// gl3_decode_kernels.h — hand-written gfx950 kernels for the single-token decode step.
//
// Replaces the TornadoVM-JITted Java kernels of
//   J/tornadovm/kernels/TransformerComputeKernelsLayered.java (fusedQKVMatmulQ8 :3038-3223,
//   matrixVectorGenericWithResidualQ8_0Byte :2888-2906, fullyFusedRmsNormFFNGateUpQ8 :3386-3549,
//   processHeadsFlashAttention :784-906, ropeRotationWithCacheCopy :495-542) and
//   J/tornadovm/kernels/TransformerComputeKernels.java (convertQ8_0toFP32 :95-126, reductionOneBlock* :149-208)
// but reproduces the ARITHMETIC of the pure-Java CPU path (the parity oracle) BIT FOR BIT:
//   * Q8_0 matvec = dotQ8Activation (J/tensor/standard/Q8_0FloatTensor.java:90-123): activation quantised to
//     int8 per 32-block (amax/127, f16-rounded scale, round-half-away), int8 x int8 -> int32 (v_dot4_i32_i8),
//     p_b = isum * (wScale * aScale) in f32, and result += p_b STRICTLY IN BLOCK ORDER;
//   * every other reduction (RMSNorm sum of squares, q.k dot, softmax denominator, weighted V sum) is also
//     evaluated in the reference's left-to-right order with one f32 rounding per step, no FMA contraction
//     (-ffp-contract=off); exp / sqrt are evaluated in double and cast, as java.lang.Math does.
// Why bit-exact and not "close": the reference re-quantises activations to int8 before every matmul, so a
// 1-ulp difference in any f32 sum flips an int8 somewhere and grows to ~1e-2 in the logits within a layer
// (measured).  Only the same summation order meets the 1e-3 north-star tolerance.
//
// In-order sums at HBM speed: v_mfma_f32_16x16x4_f32 with B = 1.0 is bit-identical to four sequential f32
// adds per row (D = fl(A[k] + D), k ascending; verified on MI355X by scripts/probes/mfma_chain_probe.hip), so
// a wavefront advances 16 rows x 4 blocks of the strictly ordered block sum per instruction on the otherwise
// idle matrix pipe.
//
// Weight layout in HBM ("Q8T", built once at upload by repack_q8t_kernel): rows are grouped in strips of 16
// and 32-element blocks in groups of 4; tile (strip, g) holds 64 blocks, lane l = (row l&15, block 4g + l>>4):
//   [64 x f16 scale][64 x 16 B quants 0..15][64 x 16 B quants 16..31]      (2176 B = 64 GGUF blocks)
// = exactly the A-operand layout of the 16x16x4 MFMA, read with three fully coalesced loads per wavefront.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gl3_seqsum.h"

namespace gl3 {

constexpr int TILE_BYTES = 2176;       // 64 Q8_0 blocks
constexpr int MV_AUX = 4;               // wavefronts running the prologue; the first one then runs the ordered sums
// NPW = wavefronts streaming weights: 4, or 8 for matrices with <= MV_WIDE_STRIPS strips (wo / down), where only one workgroup
// lands on a CU and four wavefronts cannot keep enough bytes in flight (each alternates issue -> wait -> dot).
constexpr int MV_WIDE_STRIPS = 256;
__host__ __device__ constexpr int mv_threads(int npw) { return 64 * (npw + MV_AUX); }

enum { PRO_RMS = 0, PRO_QUANT = 1 };
enum { EPI_STORE = 0, EPI_RESID = 1, EPI_SWIGLU = 2 };
// tiles a producer wavefront keeps in flight, and the tile groups all producers of a workgroup finish as one batch: the segment of the
// ordered block sum the chain wavefront adds under the next batch's stream (matvec_q8t_kernel<.., SEGS = true>).  A strip of at most
// one segment has nothing to overlap: the launch code picks SEGS = false for it, which is the one-pass chain.
__host__ __device__ constexpr int mv_ch(int epi) { return epi == EPI_SWIGLU ? 4 : 8; }
__host__ __device__ constexpr int mv_seg_groups(int npw, int epi) { return npw * mv_ch(epi); }

typedef float v4f __attribute__((ext_vector_type(4)));

#ifdef GL3_MV_TIMING
__device__ long long gl3_mv_stamp[32];
#define ATT_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) gl3_mv_stamp[i] = wall_clock64(); } while (0)
#define MV_STAMP(i, cond) do { if (blockIdx.x == 0 && (cond)) gl3_mv_stamp[i] = clock64(); } while (0)
#define PV_T(...) __VA_ARGS__
// Per-workgroup stamps of matvec_q8t_kernel on the chip-wide 100 MHz clock (clock64 is only comparable inside one workgroup): the LATEST
// time any wavefront of workgroup blockIdx.x passed slot s.  Slots: 0 start, 1 products of the last strip done, 2 last chain (segment)
// begin, 3 chain end, 4 result stored.  The host zeroes the array before a launch (scripts/probes/matvec_stamp_probe.hip).
constexpr int MV_WG_STAMPS = 1024;
__device__ unsigned long long gl3_mv_wg_stamp[MV_WG_STAMPS][8];
// MV_WG_TIME reads the clock into a register; MV_WG_PUT files it later, so that no global access stands in front of a barrier.
#define MV_WG_TIME(v) v = (unsigned long long)wall_clock64()
#define MV_WG_PUT(s, v, cond) do { if (blockIdx.x < MV_WG_STAMPS && blockIdx.y == 0 && (cond)) atomicMax(&gl3_mv_wg_stamp[blockIdx.x][s], v); } while (0)
#else
#define PV_T(...)
#define MV_STAMP(i, cond)
#define MV_WG_TIME(v)
#define MV_WG_PUT(s, v, cond)
#define ATT_STAMP(i)
#endif

// ---------------------------------------------------------------------------------------------------
// Tensor-parallel hand-over folded into the kernels that produce / consume a gathered buffer (protocol: gl3_tp.hip, "folded
// gathers").  A producer (attention -> xb, gate/up -> hb, down -> x) stores every result element into its own arena AND into each
// peer's arena (the same arena offset: own address + delta[j]); the wavefront that finishes last publishes "gather k of this buffer
// from rank me is complete" into every peer's flag word.  A consumer waits until every peer's flag for the buffer has reached k —
// in a one-wavefront wait kernel in front of it, or in its own prologue (TpRec.w inside matvec_q8t_kernel<.., TPF = true>).
// k = (step - 1) * mul + add: step = decode steps taken by this plan (device word, bumped by the embedding kernel), mul = gathers of
// the buffer per step, add = index of this gather inside the step: nothing of it is baked into a captured graph.
constexpr int TPF_MAX_PEERS = 15;
struct TpWait {
    const uint32_t* flags;       // own arena: flags[rank] of the awaited buffer; NULL = nothing to wait for
    const uint32_t* step;
    uint32_t* err;               // host-pinned word: set to 1 on a timeout
    int mul, add, tp, me;
    unsigned spin_limit;
};
struct TpPush {
    uint32_t* ticket;            // own arena: wavefronts of the producing launch that have finished
    const uint32_t* step;
    int mul, add, npeers;        // npeers = 0: nothing to push
    long delta[TPF_MAX_PEERS];   // peer arena base - own arena base (bytes), peers in rotated order (me + 1, me + 2, ...)
    uint32_t* flag[TPF_MAX_PEERS];   // peer j's flags[me] of the buffer
};
struct TpRec { TpWait w; TpPush p; };

// every lane of the calling wavefront returns once all peers have published gather k (lane p polls the flag of rank p)
__device__ __forceinline__ void tp_wait(const TpWait& w) {
    const uint32_t need = (__hip_atomic_load(w.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1u) * (uint32_t)w.mul + (uint32_t)w.add;
    const int lane = threadIdx.x & 63;
    const bool mine = lane < w.tp && lane != w.me;
    unsigned spins = 0;
    for (;;) {
        // signed distance: a peer may already be a step ahead
        const bool ok = !mine || (int32_t)(__hip_atomic_load(w.flags + (mine ? lane : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - need) >= 0;
        if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
        __builtin_amdgcn_s_sleep(8);
        if (++spins > w.spin_limit) { if (lane == 0) __hip_atomic_store(w.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");      // system scope: nothing read before the peers' data landed survives
}
// one result element into every peer's copy of the buffer
__device__ __forceinline__ void tp_push_store(const TpPush& p, float* own, float v) {
    for (int j = 0; j < p.npeers; ++j)
        *reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(own) + p.delta[j]) = v;
}
// called by every storing wavefront of the launch after its last tp_push_store (all lanes); total = such wavefronts in the launch
__device__ __forceinline__ void tp_publish(const TpPush& p, unsigned total) {
    // This wavefront's stores have been acknowledged by the peers' memory: the arenas are uncached on both sides, so a completed
    // store is a visible one and no cache needs writing back here.  (A system-scope fence per wavefront — hundreds per launch, each
    // an L2 write-back — made the folded decode step 20 % slower than the gather kernels between two ranks on one GPU.)  The one
    // wavefront that publishes fences once.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if ((threadIdx.x & 63) != 0) return;
    const unsigned ticket = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != total - 1) return;
    __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t k = (__hip_atomic_load(p.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1u) * (uint32_t)p.mul + (uint32_t)p.add;
    __threadfence_system();
    for (int j = 0; j < p.npeers; ++j) __hip_atomic_store(p.flag[j], k, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The wait as its own launch (one wavefront): the default consumer side — it cannot starve a peer rank's producer of compute units
// when ranks share one GPU (CI), which a consumer that fills the chip while it polls can.
static __global__ __launch_bounds__(64) void tp_wait_kernel(const TpRec* r) { tp_wait(r->w); }

struct MatvecArgs {
    const uint8_t* w;        // Q8T tiles
    const uint8_t* w2;       // second matrix (EPI_SWIGLU: w = gate W1, w2 = up W3)
    int rows;                // valid output rows
    int k;                   // input length (multiple of 32)
    int ng;                  // tile groups per strip = padded blocks / 4
    int nstrips;             // 16-row strips
    const float* x;          // input vector f32[k]
    const float* norm_w;     // PRO_RMS: RMSNorm weight f32[k]
    float eps;
    float* out;              // EPI_STORE: out[row]; EPI_SWIGLU: hb[row]; EPI_RESID: out[row] = resid_in[row] + acc
    const float* resid_in;   // may be NULL (tensor-parallel ranks > 0)
    float out_scale;         // EPI_STORE / EPI_RESID: the row result is multiplied by this first (1 except Granite: residualScale after wo /
                             // down, logitScale on the logits — InferenceCore.forwardGranite :893-894, :911-912, :921; x * 1.0f is exact)
    const struct MoeSlots* moe;   // SEL instantiations only (Qwen2-MoE): what each blockIdx.y slot of the launch works on
    const TpRec* tp;         // tensor parallel, folded gathers: what this launch pushes to the peers / waits for (NULL: nothing)
};

// Qwen2-MoE launches of matvec_q8t_kernel<.., SEL = true> (InferenceCore.matmulExpert :430-432): blockIdx.y = slot.  Slots j < n_sel
// are the top-k selection: the launch works on expert sel[j] of a stacked tensor — w / w2 += sel[j] * sel_stride bytes,
// x += j * x_slot_stride floats (the slot's own hbE for the down projection), out += j * out_slot_stride floats.  Slots >= n_sel
// (gate/up launch only) are chunk c = slot - n_sel of the SHARED expert's dense matrices sh_w / sh_w2: `rows` rows per chunk out of
// sh_rows, result to sh_out + c * rows — the shared expert rides in the routed experts' launch.  One record per (layer, launch) in
// device memory, written once at plan creation.
struct MoeSlots {
    const int* sel;
    size_t sel_stride;
    int x_slot_stride, out_slot_stride;
    int n_sel, sh_rows;
    const uint8_t* sh_w;
    const uint8_t* sh_w2;
    float* sh_out;
};

// Workgroup barrier for LDS hand-overs: s_waitcnt lgkmcnt(0) + s_barrier.  __syncthreads() also waits for vmcnt(0) — every global load
// a wavefront has in flight — which turns a prefetch issued in front of it into a full memory round trip per barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

struct LdsBarrier { __device__ __forceinline__ void operator()() const { lds_barrier(); } };      // Sync functor of exact_seqsum_lds

__device__ __forceinline__ float h2f(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// Strict left-to-right f32 sum of n floats held in LDS, executed redundantly by every lane of the calling
// wavefront (uniform addresses -> LDS broadcast).  SQ = true sums x*x (InferenceCore.rmsnorm :41).
template <bool SQ>
__device__ __forceinline__ float seq_add4(float s, const float4& a) {
    if (SQ) { s = s + a.x * a.x; s = s + a.y * a.y; s = s + a.z * a.z; s = s + a.w * a.w; }
    else { s = s + a.x; s = s + a.y; s = s + a.z; s = s + a.w; }
    return s;
}
template <bool SQ>
__device__ __forceinline__ float seq_sum_lds(const float* v, int n, float start = 0.f) {     // start: running sum before v[0] (chunked rows)
    float s = start;
    int i = 0;
    if (n >= 16) {                                     // software pipeline: the next 8 elements are in flight
        float4 a0 = *reinterpret_cast<const float4*>(v), a1 = *reinterpret_cast<const float4*>(v + 4);
        for (; i + 16 <= n; i += 8) {
            const float4 b0 = *reinterpret_cast<const float4*>(v + i + 8), b1 = *reinterpret_cast<const float4*>(v + i + 12);
            s = seq_add4<SQ>(s, a0); s = seq_add4<SQ>(s, a1);
            a0 = b0; a1 = b1;
        }
        s = seq_add4<SQ>(s, a0); s = seq_add4<SQ>(s, a1);
        i += 8;
    }
    for (; i + 4 <= n; i += 4) s = seq_add4<SQ>(s, *reinterpret_cast<const float4*>(v + i));
    for (; i < n; ++i) s = SQ ? s + v[i] * v[i] : s + v[i];
    return s;
}

// a * b as one v_mul_f32 the SLP vectoriser cannot pair: v_pk_mul_f32 wants its operands in aligned register pairs, and the
// v_mov shuffles it inserts for that read freshly issued LDS results, i.e. wait for them — which is what a read ring is there to avoid.
__device__ __forceinline__ float mul_f32_scalar(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// seq_sum_lds<false> with the LDS reads three 16-element groups ahead of the adds, pinned there with sched_barrier (the scheduler
// otherwise sinks every read next to its use and the chain waits an LDS round trip per group: 11 cycles per element instead of ~6,
// scripts/probes/seqsum_time.hip).  Same adds in the same order.  v may differ per lane (lane = row) or be uniform.
__device__ __forceinline__ float seq_sum_lds_ring(const float* v, int n, float start = 0.f) {
    float s = start;
    const int G = n >> 4;
    int i = 0;
    if (G >= 3) {
        float4 a0, a1, a2, a3, b0, b1, b2, b3, c0, c1, c2, c3;
#define SSR_LD(G_, V0_, V1_, V2_, V3_) do { const float* q_ = v + 16 * min((G_), G - 1); V0_ = *reinterpret_cast<const float4*>(q_); \
        V1_ = *reinterpret_cast<const float4*>(q_ + 4); V2_ = *reinterpret_cast<const float4*>(q_ + 8); V3_ = *reinterpret_cast<const float4*>(q_ + 12); } while (0)
#define SSR_ADD(V0_, V1_, V2_, V3_) do { s = seq_add4<false>(s, V0_); s = seq_add4<false>(s, V1_); s = seq_add4<false>(s, V2_); s = seq_add4<false>(s, V3_); } while (0)
        SSR_LD(0, a0, a1, a2, a3); SSR_LD(1, b0, b1, b2, b3); SSR_LD(2, c0, c1, c2, c3);
        int g = 0;
        for (; g + 3 <= G; g += 3) {
            SSR_ADD(a0, a1, a2, a3); SSR_LD(g + 3, a0, a1, a2, a3); __builtin_amdgcn_sched_barrier(0);
            SSR_ADD(b0, b1, b2, b3); SSR_LD(g + 4, b0, b1, b2, b3); __builtin_amdgcn_sched_barrier(0);
            SSR_ADD(c0, c1, c2, c3); SSR_LD(g + 5, c0, c1, c2, c3); __builtin_amdgcn_sched_barrier(0);
        }
        if (g < G) { SSR_ADD(a0, a1, a2, a3); ++g; }
        if (g < G) { SSR_ADD(b0, b1, b2, b3); ++g; }
#undef SSR_ADD
#undef SSR_LD
        i = 16 * G;
    }
    for (; i + 4 <= n; i += 4) s = seq_add4<false>(s, *reinterpret_cast<const float4*>(v + i));
    for (; i < n; ++i) s = s + v[i];
    return s;
}

// ---------------------------------------------------------------------------------------------------
// Activation quantisation into LDS (Q8_0FloatTensor.java:96-118): 8 consecutive threads own one 32-block.
// xq[32*b ..] = int8 quants of block b, xs[b] = f16-rounded activation scale.  v = value already normalised.
// the 4 packed quants of a quad and its block's scale (valid in all 8 lanes of the block)
__device__ __forceinline__ uint32_t quantize_quad_pack(float4 v, float& qs_out) {
    float amax = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
    // maximum over the block's 8 lanes with DPP moves (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror) instead of
    // three dependent ds_bpermute round trips through LDS (__shfl_xor): ~300 cycles less per quad on the prologue's critical path
    amax = fmaxf(amax, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, amax), 0xB1, 0xf, 0xf, false)));
    amax = fmaxf(amax, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, amax), 0x4E, 0xf, 0xf, false)));
    amax = fmaxf(amax, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, amax), 0x141, 0xf, 0xf, false)));
    const float qs = amax / 127.0f;
    const float ainv = qs != 0.f ? 1.0f / qs : 0.f;
    const float s0 = v.x * ainv, s1 = v.y * ainv, s2 = v.z * ainv, s3 = v.w * ainv;
    const int q0 = (int)(s0 + copysignf(0.5f, s0)), q1 = (int)(s1 + copysignf(0.5f, s1));
    const int q2 = (int)(s2 + copysignf(0.5f, s2)), q3 = (int)(s3 + copysignf(0.5f, s3));
    qs_out = (float)(_Float16)qs;                                        // float16ToFloat(floatToFloat16(qs))
    return (uint32_t)(q0 & 0xFF) | ((uint32_t)(q1 & 0xFF) << 8) | ((uint32_t)(q2 & 0xFF) << 16) | ((uint32_t)(q3 & 0xFF) << 24);
}

__device__ __forceinline__ void quantize_quad(float4 v, int qd, uint8_t* xq, float* xs) {
    float qs;
    const uint32_t packed = quantize_quad_pack(v, qs);
    *reinterpret_cast<uint32_t*>(xq + 4 * qd) = packed;                  // byte 32*b + 4*(qd&7)
    if ((qd & 7) == 0) xs[qd >> 3] = qs;
}

// Small-batch operand layout (gl3_bd_gemm.h): byte offset of quad qd (elements 4qd .. 4qd + 3 of a token's row) in XQ2, and
// float offset of block blk's scale in XS2; tslots token slots.
__device__ __forceinline__ size_t bdq_offset(int qd, int tok, int tslots) {
    const int blk = qd >> 3, qi = qd & 7, c = qi >> 1;
    const int g = ((c & 1) << 1) | (c >> 1);                 // k-chunk 0, 1, 2, 3 -> k-group 0, 2, 1, 3
    return ((size_t)(blk >> 1) * tslots + tok) * 64 + 16 * g + 8 * (blk & 1) + 4 * (qi & 1);
}
__device__ __forceinline__ size_t bds_offset(int blk, int tok, int tslots) { return ((size_t)(blk >> 2) * tslots + tok) * 4 + (blk & 3); }

__device__ __forceinline__ int dot32(const int4& a0, const int4& a1, const int4& b0, const int4& b1) {
    int s = 0;
    s = __builtin_amdgcn_sdot4(a0.x, b0.x, s, false); s = __builtin_amdgcn_sdot4(a0.y, b0.y, s, false);
    s = __builtin_amdgcn_sdot4(a0.z, b0.z, s, false); s = __builtin_amdgcn_sdot4(a0.w, b0.w, s, false);
    s = __builtin_amdgcn_sdot4(a1.x, b1.x, s, false); s = __builtin_amdgcn_sdot4(a1.y, b1.y, s, false);
    s = __builtin_amdgcn_sdot4(a1.z, b1.z, s, false); s = __builtin_amdgcn_sdot4(a1.w, b1.w, s, false);
    return s;
}

template <bool NT>
__device__ __forceinline__ int4 ld16(const uint8_t* p) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    v4i v;
    if (NT) v = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(p));
    else v = *reinterpret_cast<const v4i*>(p);
    int4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w;
    return r;
}
template <bool NT>
__device__ __forceinline__ uint16_t ld2(const uint8_t* p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p));
    return *reinterpret_cast<const uint16_t*>(p);
}

// ---------------------------------------------------------------------------------------------------
// Dequant-fused Q8_0 matvec, bit-exact to FloatTensor.matmul + dotQ8Activation.
// Workgroup = 8 wavefronts with three roles:
//   producers (waves 0-3): stream the weight tiles of the workgroup's 16-row strips (lane = one 32-block of one
//       row: 3 coalesced non-temporal loads, 8 v_dot4, p = isum*(wScale*aScale)) into a double-buffered LDS
//       array.  Their first loads are issued BEFORE the activation is ready, so HBM latency hides the prologue;
//   aux (waves 4-7): the prologue — RMSNorm with the exact in-order sum of squares (gl3_seqsum.h) and the
//       Q8_0 activation quantisation into LDS; waves 5-7 then retire;
//   chain (wave 4): adds the p's of each row in block order with v_mfma_f32_16x16x4_f32 (B = 1.0) and applies
//       the epilogue while the producers already stream the next strip.
// SEGS = true (picked by the launch code for strips of more than one segment, mv_seg_groups): the chain runs in segments under the
// weight stream.  What the producers finish as one batch (NPW wavefronts x CH tiles = SEG groups, contiguous in K) is handed over at a
// workgroup barrier (lds_barrier: no vmcnt(0)), and the chain wavefront adds segment s while segment s + 1 streams; acc runs on across
// the segments, so the adds and their order are those of one pass over the strip.  Every wavefront meets the barrier
// ceil(ceil(ng / NPW) / CH) times per strip, also one whose tiles end a batch early.  Behind the last byte of a workgroup's last strip
// only the last segment's adds and the epilogue remain (down at K = 14336: 48 of 112 groups, gate/up at K = 4096: 16 of 32).
// SEGS = false is the one-pass chain behind one __syncthreads() per strip: for strips of one segment (qkv, wo, logits at K = 4096,
// every matrix of Llama-3.2-1B) the segment barrier form measured 0.05 us slower per launch and buys nothing.  Figures per class in
// profiles/matvec_chain_overlap.md; one barrier round costs about 0.05 us, one group of the chain about 0.018 us.
// Register pressure is the maximum of the roles, not their sum (wave-uniform branches).
//   LDS: xq[ng*128] | xs[ng*4] f32 | xf[k + 32] f32 (PRO_RMS) | pbuf[2][NM][ng*64] f32 | red[4] | sync[4]
// TPF (tensor parallel, folded gathers): the aux wavefronts wait for the peers' slices of x before they read it (after the barrier
// that releases the producers: the weight stream starts while the wait polls), and the chain wavefront stores every result into
// the peers' arenas as well and publishes the gather (TpRec above).
template <int PRO, int EPI, int NPW = 4, bool SEL = false, bool TPF = false, bool SEGS = false>
__global__ __launch_bounds__(mv_threads(NPW), NPW == 4 ? 4 : 2) void matvec_q8t_kernel(const MatvecArgs a_in) {
    MatvecArgs a = a_in;
    if (SEL) {                                          // wave-uniform: one scalar load of the expert id
        const int slot = blockIdx.y;
        const MoeSlots m = *a.moe;
        if (slot < m.n_sel) {
            const size_t woff = (size_t)m.sel[slot] * m.sel_stride;
            a.w += woff;
            if (a.w2) a.w2 += woff;
            a.x += (size_t)slot * m.x_slot_stride;
            a.out += (size_t)slot * m.out_slot_stride;
        } else {
            const int c = slot - m.n_sel;
            const size_t woff = (size_t)c * m.sel_stride;
            a.w = m.sh_w + woff;
            a.w2 = m.sh_w2 ? m.sh_w2 + woff : nullptr;
            a.out = m.sh_out + (size_t)c * a.rows;
            const int left = m.sh_rows - c * a.rows;
            if (left < a.rows) { a.rows = left; a.nstrips = (left + 15) / 16; }
        }
    }
    constexpr int MV_PRODUCERS = NPW;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int NM = (EPI == EPI_SWIGLU) ? 2 : 1;
    constexpr int CH = mv_ch(EPI);                    // tiles in flight per producer wave
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nb4 = a.ng * 4;
    constexpr int SEG = mv_seg_groups(NPW, EPI);       // groups per chain segment = what the producers finish as one batch (contiguous in K)
    const int nbatch = SEGS ? ((a.ng + NPW - 1) / NPW + CH - 1) / CH : 1;      // barrier rounds per strip, the same for every wavefront
    uint8_t* xq = smem;
    float* xs = reinterpret_cast<float*>(smem + (size_t)nb4 * 32);
    float* xf = xs + nb4;
    float* pbuf = xf + (PRO == PRO_RMS ? a.k + 32 : 0);     // 32 zero floats pad xf for exact_sumsq_lds
    float* red = pbuf + (size_t)2 * NM * a.ng * 64;         // [0] plain-chain result
    int* sync_w = reinterpret_cast<int*>(red + 4);          // [0] aux sub-barrier counter, [1] activation-ready flag
    const size_t strip_bytes = (size_t)a.ng * TILE_BYTES;
    MV_STAMP(0, t == 0);
    PV_T(unsigned long long wg_t0 = 0, wg_t1 = 0, wg_t2 = 0;)
    MV_WG_TIME(wg_t0);
    if (t < 2) sync_w[t] = 0;

    if (wave < MV_PRODUCERS) {
        // ------------------------------------------------------------------ producers
        const int nt = (a.ng - wave + MV_PRODUCERS - 1) / MV_PRODUCERS;      // tiles g = wave + 4*i of a strip
        uint16_t sc[NM][CH];
        int4 lo[NM][CH], hi[NM][CH];
        auto issue = [&](int strip, int i0) {
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                if (i0 + u < nt) {
                    const int g = wave + (i0 + u) * MV_PRODUCERS;
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const uint8_t* p = (m == 0 ? a.w : a.w2) + (size_t)strip * strip_bytes + (size_t)g * TILE_BYTES;
                        sc[m][u] = ld2<true>(p + 2 * lane);
                        lo[m][u] = ld16<true>(p + 128 + 16 * lane);
                        hi[m][u] = ld16<true>(p + 1152 + 16 * lane);
                    }
                }
            }
        };
        auto compute = [&](int i0, float* pb) {
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                if (i0 + u < nt) {
                    const int g = wave + (i0 + u) * MV_PRODUCERS;
                    const int xb = 4 * g + (lane >> 4);
                    const int4 xlo = *reinterpret_cast<const int4*>(xq + 32 * xb);
                    const int4 xhi = *reinterpret_cast<const int4*>(xq + 32 * xb + 16);
                    const float xsc = xs[xb];
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const int isum = dot32(lo[m][u], hi[m][u], xlo, xhi);
                        pb[(size_t)m * a.ng * 64 + g * 64 + lane] = (float)isum * (h2f(sc[m][u]) * xsc);
                    }
                }
            }
        };
        int strip = blockIdx.x;
        __syncthreads();                                         // the only prologue barrier the producers join
        if (strip < a.nstrips) issue(strip, 0);                  // HBM latency hides the activation prologue
        while (__hip_atomic_load(&sync_w[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) __builtin_amdgcn_s_sleep(2);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        MV_STAMP(3, t == 0);
        int it = 0;
        for (; strip < a.nstrips; strip += gridDim.x, ++it) {
            float* pb = pbuf + (size_t)(it & 1) * NM * a.ng * 64;
            // batch i0 / CH = groups [i0 / CH * SEG, (i0 / CH + 1) * SEG) of the strip: one chain segment
            for (int i0 = 0; i0 < nt; i0 += CH) {
                if (it != 0 || i0 != 0) issue(strip, i0);
                compute(i0, pb);
                if (SEGS) {
                    MV_STAMP(4 + 2 * it, t == 0 && it < 4 && i0 + CH >= nt);
                    MV_WG_TIME(wg_t1);
                    lds_barrier();                               // hands the segment to the chain wavefront; no vmcnt(0) as __syncthreads() has
                }
            }
            if (SEGS) {
                // a wavefront whose tiles end a batch early (ng % NPW != 0) still meets the others once per batch
                for (int b = (nt + CH - 1) / CH; b < nbatch; ++b) lds_barrier();
            } else {
                MV_STAMP(4 + 2 * it, t == 0 && it < 4);
                MV_WG_TIME(wg_t1);
                __syncthreads();
            }
            MV_STAMP(5 + 2 * it, t == 0 && it < 4);
        }
        MV_WG_PUT(0, wg_t0, t == 0); MV_WG_PUT(1, wg_t1, lane == 0);
        return;
    }

    // ---------------------------------------------------------------------- aux waves: prologue
    // the prologue is the critical path of the kernel; the producers only issue their loads and poll
    __builtin_amdgcn_s_setprio(3);
    const int ta = t - 64 * MV_PRODUCERS;                // 0..255
    const int nquads = a.k >> 2;
    float scale = 1.0f;
    constexpr int NXV = (PRO == PRO_RMS) ? 5 : 14;       // quads of the activation held in registers per aux thread
    float4 nwv[5], xv[NXV];                              // this thread's RMSNorm weights and activations
    // all activation loads first: they come from L2, the norm weights behind them from HBM (vmcnt retires in order, and the
    // activation is needed 5 us before the weights)
    // UNCONDITIONAL loads with clamped indices (quads past the end re-read the last one: an L1 hit that is never used).  With a
    // lane-predicated `if (qd < nquads) xv[i] = load`, and even with a wave-uniform condition, the compiler waited
    // (s_waitcnt vmcnt(0)) after every single load: 10 to 14 serial L2 round trips in front of every matvec (seen in the ISA).
    if (!TPF) {
#pragma unroll
        for (int i = 0; i < NXV; ++i) xv[i] = *reinterpret_cast<const float4*>(a.x + 4 * min(ta + 256 * i, nquads - 1));
    }
    if (PRO == PRO_RMS) {
#pragma unroll
        for (int i = 0; i < 5; ++i) nwv[i] = *reinterpret_cast<const float4*>(a.norm_w + 4 * min(ta + 256 * i, nquads - 1));
    }
    __syncthreads();                                     // activation loads are queued ahead of the weight stream
    if (TPF) {
        if (a.tp->w.flags) tp_wait(a.tp->w);
#pragma unroll
        for (int i = 0; i < NXV; ++i) xv[i] = *reinterpret_cast<const float4*>(a.x + 4 * min(ta + 256 * i, nquads - 1));
    }
    SubBarrier aux_sync{&sync_w[0], MV_AUX, 0};
    for (int b = (a.k >> 5) + ta; b < nb4; b += 256) {   // zero-padded blocks: nothing of them waits for the sum
        xs[b] = 0.f;
        const int4 z = {0, 0, 0, 0};
        *reinterpret_cast<int4*>(xq + 32 * b) = z;
        *reinterpret_cast<int4*>(xq + 32 * b + 16) = z;
    }
    if (PRO == PRO_RMS) {
        if (nquads <= NXV * 256) {
#pragma unroll
            for (int i = 0; i < NXV; ++i) { const int qd = ta + 256 * i; if (qd < nquads) *reinterpret_cast<float4*>(xf + 4 * qd) = xv[i]; }
        } else {
            for (int qd = ta; qd < nquads; qd += 256)
                *reinterpret_cast<float4*>(xf + 4 * qd) = *reinterpret_cast<const float4*>(a.x + 4 * qd);
        }
        if (ta < 32) xf[a.k + ta] = 0.f;
        aux_sync();
        MV_STAMP(1, ta == 0);
        // InferenceCore.rmsnorm :41 — the strict left-to-right sum of squares, evaluated exactly in parallel
        // (gl3_seqsum.h); pbuf is free during the prologue and serves as its scratch.
        float ss;
        if ((size_t)2 * NM * a.ng * 64 * 4 >= ss_scratch_bytes(a.k) && a.k >= 1024 && a.k <= 5120) {
            ss = exact_sumsq_lds(xf, a.k, reinterpret_cast<uint8_t*>(pbuf), ta, aux_sync);
        } else {
            if (wave == MV_PRODUCERS) {
                const float s1 = seq_sum_lds<true>(xf, a.k);
                if (lane == 0) red[0] = s1;
            }
            aux_sync();
            ss = red[0];
        }
        MV_STAMP(2, ta == 0);
        ss /= (float)a.k;
        ss += a.eps;
        scale = (float)(1.0 / sqrt((double)ss));
    }
    if (nquads <= NXV * 256) {
#pragma unroll
        for (int i = 0; i < NXV; ++i) {
            const int qd = ta + 256 * i;
            if (qd < nquads) {
                float4 v = xv[i];
                if (PRO == PRO_RMS) {
                    const float4 w = nwv[i];
                    v.x = w.x * (scale * v.x); v.y = w.y * (scale * v.y); v.z = w.z * (scale * v.z); v.w = w.w * (scale * v.w);
                }
                quantize_quad(v, qd, xq, xs);
            }
        }
    } else {
        for (int qd = ta; qd < nquads; qd += 256) {
            float4 v = *reinterpret_cast<const float4*>(a.x + 4 * qd);
            if (PRO == PRO_RMS) {
                const float4 w = *reinterpret_cast<const float4*>(a.norm_w + 4 * qd);
                v.x = w.x * (scale * v.x); v.y = w.y * (scale * v.y); v.z = w.z * (scale * v.z); v.w = w.w * (scale * v.w);
            }
            quantize_quad(v, qd, xq, xs);
        }
    }
    aux_sync();                                          // xq / xs complete
    if (ta == 0) __hip_atomic_store(&sync_w[1], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (wave != MV_PRODUCERS) return;                    // waves 5-7 retire; wave 4 becomes the chain wavefront

    // ---------------------------------------------------------------------- chain wavefront
    int it = 0;
    for (int strip = blockIdx.x; strip < a.nstrips; strip += gridDim.x, ++it) {
        const float* pb = pbuf + (size_t)(it & 1) * NM * a.ng * 64;
        v4f acc[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[m] = (v4f){0.f, 0.f, 0.f, 0.f};
        // One segment per producer batch: segment s is summed while the producers stream segment s + 1 (or the next strip), acc runs
        // on across the segments, so the order of the adds is the one of a single pass over the strip.
        for (int b = 0; b < nbatch; ++b) {
            if (SEGS) lds_barrier(); else __syncthreads();      // segment b of this strip (SEGS = false: the whole strip) is in pbuf
            MV_STAMP(16 + 2 * it, lane == 0 && it < 4 && b == nbatch - 1);
            MV_WG_TIME(wg_t1);
            int g = b * SEG;
            const int ge = SEGS ? min(g + SEG, a.ng) : a.ng;
            for (; g + 8 <= ge; g += 8) {             // result += p_b, b ascending: 4 blocks x 16 rows per MFMA
                float av[NM][8];
#pragma unroll
                for (int m = 0; m < NM; ++m)
#pragma unroll
                    for (int u = 0; u < 8; ++u) av[m][u] = pb[(size_t)m * a.ng * 64 + (g + u) * 64 + lane];
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int m = 0; m < NM; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][u], 1.0f, acc[m], 0, 0, 0);
            }
            for (; g < ge; ++g)
#pragma unroll
                for (int m = 0; m < NM; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(pb[(size_t)m * a.ng * 64 + g * 64 + lane], 1.0f, acc[m], 0, 0, 0);
        }
        MV_STAMP(17 + 2 * it, lane == 0 && it < 4);
        MV_WG_TIME(wg_t2);
        // D[i][j]: row i = 4*(lane>>4) + reg, all 16 columns identical.  Lane l takes row (l & 3) of its own group
        // when (l & 15) < 4, so the 16 rows of the strip are finished by 16 lanes in parallel (one double exp each).
        if ((lane & 15) < 4) {
            const int r = lane & 3;
            const int row = strip * 16 + 4 * (lane >> 4) + r;
            if (row < a.rows) {
                const float v0 = r == 0 ? acc[0][0] : r == 1 ? acc[0][1] : r == 2 ? acc[0][2] : acc[0][3];
                float res;
                if (EPI == EPI_STORE) res = v0 * a.out_scale;
                if (EPI == EPI_RESID) res = a.resid_in ? a.resid_in[row] + v0 * a.out_scale : v0 * a.out_scale;
                if (EPI == EPI_SWIGLU) {                  // InferenceCore.java:155-158, exp in double
                    const float v1 = r == 0 ? acc[NM - 1][0] : r == 1 ? acc[NM - 1][1] : r == 2 ? acc[NM - 1][2] : acc[NM - 1][3];
                    const float gte = v0 / (float)(1.0 + exp(-(double)v0));
                    res = gte * v1;
                }
                a.out[row] = res;
                if (TPF) tp_push_store(a.tp->p, a.out + row, res);
            }
        }
        PV_T(asm volatile("s_waitcnt vmcnt(0)" ::: "memory");)
        MV_WG_TIME(wg_t0);
        MV_WG_PUT(2, wg_t1, lane == 0); MV_WG_PUT(3, wg_t2, lane == 0); MV_WG_PUT(4, wg_t0, lane == 0);
    }
    if (TPF && a.tp->p.npeers) tp_publish(a.tp->p, gridDim.x);
}

// ---------------------------------------------------------------------------------------------------
// Embedding row gather + dequant: x[i] = q * d  (token_embedding_table.copyTo, InferenceCore.java:61;
// replaces the host row copy of forwardTornadoVM :956-980 + convertQ8_0toFP32).
// tp (folded gathers): the kernel opens decode step number *step + 1 of the plan — it first waits until the peers' last pushes of
// the previous step into x have landed (a later arrival would overwrite this step's embedding), then bumps the step word.
static __global__ __launch_bounds__(256) void embed_q8t_kernel(const uint8_t* __restrict__ emb, int ng, int dim,
                                                         const int* __restrict__ dyn, float* __restrict__ x, float emb_scale,
                                                         const TpRec* tp = nullptr, uint32_t* step = nullptr) {
    if (step) {
        const uint32_t s = *step;
        __syncthreads();
        if (threadIdx.x == 0) *step = s + 1;
        if (tp) {                          // as tp_wait with "need" spelled out: the step word is being rewritten
            TpWait w = tp->w;
            const uint32_t need = s * (uint32_t)w.mul;
            const int lane = threadIdx.x & 63;
            const bool mine = lane < w.tp && lane != w.me;
            unsigned spins = 0;
            for (;;) {
                const bool ok = !mine || (int32_t)(__hip_atomic_load(w.flags + (mine ? lane : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - need) >= 0;
                if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
                __builtin_amdgcn_s_sleep(8);
                if (++spins > w.spin_limit) { if (lane == 0) __hip_atomic_store(w.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
            }
        }
    }
    const int token = dyn[0];
    const uint8_t* strip = emb + (size_t)(token >> 4) * ng * TILE_BYTES;
    const int i16 = token & 15;
    for (int i = threadIdx.x; i < dim; i += 256) {
        const int b = i >> 5, j = i & 31;
        const uint8_t* p = strip + (size_t)(b >> 2) * TILE_BYTES;
        const int l = i16 + 16 * (b & 3);
        const float d = h2f(*reinterpret_cast<const uint16_t*>(p + 2 * l));
        const int8_t q = (int8_t)p[(j < 16 ? 128 : 1152) + 16 * l + (j & 15)];
        x[i] = ((float)q * d) * emb_scale;        // Granite: embeddingScale (forwardGranite :829); 1 otherwise (exact)
    }
}

// ---------------------------------------------------------------------------------------------------
// Greedy sampling on the device: first index of the maximum (strict >), FloatTensor.argmax
// J/tensor/standard/FloatTensor.java:138-151 — NOT the strided-scan tie-break of the reference's
// argmaxLogits (TransformerComputeKernels.java:25-59).
// One launch, AMX_WGS workgroups: each scans a contiguous slice (float4 loads), publishes its (value, index) pair and takes a
// ticket; the LAST workgroup to arrive (no spinning: whoever draws the final ticket) folds the pairs in slice order and resets the
// ticket for the next token.  ws = int[2 + 2 * AMX_WGS]: [0] result, [1] ticket (zero at allocation), then the pairs.
// (One 1024-thread workgroup took 45 us for the 128256 logits of Llama-3.)
constexpr int AMX_WGS = 64;
__device__ __forceinline__ void amx_take(float& best, int& idx, float f, int i) {
    if (f > best || (f == best && i < idx)) { best = f; idx = i; }
}
static __global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ v, int n, int* __restrict__ ws) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    __shared__ int last;
    const int t = threadIdx.x, b = blockIdx.x;
    const int per = (((n + AMX_WGS - 1) / AMX_WGS) + 3) & ~3;          // slice length, multiple of 4 (n % 4 == 0 is not required)
    const int lo = b * per, hi = min(n, lo + per);
    float best = -INFINITY;
    int idx = 0x7FFFFFFF;
    const bool vec = (reinterpret_cast<uintptr_t>(v) & 15) == 0;
    if (vec) {
        for (int i = lo + 4 * t; i < hi; i += 1024) {
            if (i + 4 <= hi) {
                const float4 f = *reinterpret_cast<const float4*>(v + i);
                amx_take(best, idx, f.x, i); amx_take(best, idx, f.y, i + 1); amx_take(best, idx, f.z, i + 2); amx_take(best, idx, f.w, i + 3);
            } else {
                for (int j = i; j < hi; ++j) amx_take(best, idx, v[j], j);
            }
        }
    } else {
        for (int i = lo + t; i < hi; i += 256) amx_take(best, idx, v[i], i);
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        amx_take(best, idx, ob, oi);
    }
    if ((t & 63) == 0) { bv[t >> 6] = best; bi[t >> 6] = idx; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; ++w) amx_take(best, idx, bv[w], bi[w]);
        __hip_atomic_store(ws + 2 + 2 * b, __builtin_bit_cast(int, best), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ws + 3 + 2 * b, idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int ticket = __hip_atomic_fetch_add(ws + 1, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = ticket == AMX_WGS - 1;
    }
    __syncthreads();
    if (!last) return;
    if (t < 64) {                                   // AMX_WGS = 64 pairs: one per lane
        best = __builtin_bit_cast(float, __hip_atomic_load(ws + 2 + 2 * t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        idx = __hip_atomic_load(ws + 3 + 2 * t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int m = 32; m >= 1; m >>= 1) {
            const float ob = __shfl_xor(best, m, 64);
            const int oi = __shfl_xor(idx, m, 64);
            amx_take(best, idx, ob, oi);
        }
        if (t == 0) {
            ws[0] = idx == 0x7FFFFFFF ? 0 : idx;
            __hip_atomic_store(ws + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// One-time layout transform at upload: GGUF Q8_0 blocks (34 B: f16 d + 32 x int8, GGMLType.java:13) of rows
// [r0, r0+rows) and blocks [b0, b0+nb) of a [*, nb_full*32] matrix -> Q8T tiles.  One thread per destination
// (row, block) slot incl. zero padding (rows -> x16, blocks -> x4).
static __global__ void repack_q8t_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int nb, int ng,
                                  long r0, int b0, int nb_full) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int rows16 = (rows + 15) & ~15, nb4 = ng * 4;
    if (idx >= (long)rows16 * nb4) return;
    const int row = (int)(idx / nb4), pb = (int)(idx % nb4);
    uint8_t* tile = dst + ((size_t)(row >> 4) * ng + (pb >> 2)) * TILE_BYTES;
    const int l = (row & 15) + 16 * (pb & 3);
    uint16_t h[17];
    if (row < rows && pb < nb) {
        const uint16_t* s = reinterpret_cast<const uint16_t*>(src + ((size_t)(r0 + row) * nb_full + b0 + pb) * 34);
#pragma unroll
        for (int i = 0; i < 17; ++i) h[i] = s[i];
    } else {
#pragma unroll
        for (int i = 0; i < 17; ++i) h[i] = 0;
    }
    *reinterpret_cast<uint16_t*>(tile + 2 * l) = h[0];
    uint16_t* lo = reinterpret_cast<uint16_t*>(tile + 128 + 16 * l);
    uint16_t* hi = reinterpret_cast<uint16_t*>(tile + 1152 + 16 * l);
#pragma unroll
    for (int i = 0; i < 8; ++i) { lo[i] = h[1 + i]; hi[i] = h[9 + i]; }
}

}  // namespace gl3

#include "gl3_decode_attn.h"      // the decode attention kernels and their launch plan: every file that includes this one sees them
