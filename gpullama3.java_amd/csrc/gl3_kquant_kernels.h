// gl3_kquant_kernels.h — Q4_K / Q5_K / Q6_K matrices kept in their own bit width in HBM (GL3_FLAG_KQUANT_NATIVE) and streamed by the
// decode matvec, bit-equal to the Q8_0 path on the load-time conversion.
//
// What the default path does with a K-quant tensor (gl3_kquant_to_q8_0 = ModelLoader.dequantizeToQ8_0TornadoTensor) is a pure
// function of the 32 K-quant elements of a block: x_i = getFloat(i), max_abs = max |x_i|, scale = max_abs / 127,
// q_i = clamp(Math.round(x_i * (1 / scale)), -128, 127), stored scale = f16(scale).  The producer lane that holds those 32 elements
// rebuilds (q_i, f16 scale) in registers (kq_rebuild_q4k / kq_rebuild_q5k / kq_rebuild_q6k) and runs the int8 dot of matvec_q8t_kernel
// on them, so every product p_b = isum * (wScale * aScale), the ordered block sum and the epilogues are those of the converted plan.
//
// Layouts in HBM, built at upload by repack_q4k_kernel / repack_q5k_kernel / repack_q6k_kernel.  As in Q8T a tile is 16 rows x 4 blocks
// of 32 elements, lane l = (row l & 15, block 4g + (l >> 4)), and every field is one coalesced load of the wavefront:
//   Q4_K tile, 1216 B (19 B per block; GGUF 18, Q8T 34):
//     [16 x u32   f16 d | f16 dmin << 16 of row r: a tile lies inside one super-block of its rows]
//     [64 x u16   scale | min << 6 | qarg << 12: the block's 6-bit pair, and the nibble value at which |getFloat| peaks]
//     [64 x 16 B  nibbles: byte t of word j = element 8j + t (low nibble) | element 8j + 4 + t (high nibble)]
//   Q5_K tile, 1488 B (23.25 B per block; GGUF 22):
//     [16 x u32   f16 d | f16 dmin << 16 of row r, as Q4_K]
//     [16 x u8    bit j = bit 4 of qarg of block 4g + j of row r: scale, min and a 5-bit qarg are 17 bits, one more than the u16 below]
//     [64 x u16   scale | min << 6 | (qarg & 15) << 12]
//     [64 x u32   fifth bits: bit 8t + f = element 4f + t, so that (word >> f) & 0x01010101 lines up with the masked nibble word]
//     [64 x 16 B  low nibbles, packed as Q4_K's]
//   Q6_K tile, 1792 B (28 B per block; GGUF 26.25):
//     [64 x u32   int8 scale of elements 0..15 | int8 scale of 16..31 << 8 | f16 d << 16]
//     [64 x 8 B   high two bits: bits 2f, 2f + 1 of byte t of word h = element 16h + 4f + t]
//     [64 x 16 B  low nibbles, packed as Q4_K's]
// The nibble packing puts the four elements of one v_dot4 operand into the four bytes of one masked word, so GGUF's interleaving
// (low and high nibbles of a byte belong to different blocks) is undone once, at upload.
//
// Q4_K: a block has at most 16 distinct values x(q) = (d * sc) * q - dmin * m.  x is monotone in q (one f32 rounding per step keeps
// the order), so |x| over the nibbles present peaks at the smallest or the largest of them; which one is decided once at upload with
// the same f32 arithmetic and kept as qarg.  The lane computes max_abs = |x(qarg)|, the 16 int8 codes of q = 0..15 (4 registers),
// and turns nibbles into int8 lanes with two v_perm_b32 and a v_bfi_b32 per four elements.
// Q5_K: x(q) is Q4_K's with q = 0..31, monotone by the same argument, so max_abs = |x(qarg)| comes from the header again.  32 levels
// for 32 elements: a code table would cost what the elements cost and its lookup on top, so every element is computed where it
// stands — four 5-bit values per word from (and, shift-and-or) of the nibble word and the fifth-bit word, then per element
// v_cvt_f32_ubyteN, mul, sub, mul and the six steps of kq_round_clamp, once (Q6_K runs its elements twice), and two v_perm_b32 and an
// or to pack four codes.  About 415 VALU instructions per block: some 40 for the header (two IEEE divisions), 4 per word for the 5-bit
// values, 10 per element, 3 per word to pack.
// Q6_K: 64 levels per 16-element sub-block and two sub-blocks per block: per element (v_cvt_f32_ubyteN, sub, mul), twice — once for
// max_abs, once for the codes — rather than 32 live registers.
//
// The rebuild is a few hundred VALU instructions per 32 elements (Q4_K: 16 table entries of about ten steps, then nine per four elements,
// about 270; Q5_K: about 415; Q6_K: about a dozen per element, twice, about 475) where Q8T needs 8 v_dot4, so the kernel is sized for VALU
// throughput, not for bytes in flight:
// KQ_NPW = 12 producer wavefronts in the one workgroup a CU holds (16 wavefronts of at most 128 registers) and only two tiles in flight
// per wavefront (kq_ch): three producers per SIMD alternate between waiting and rebuilding.  (Two workgroups of 8 producers would need 80
// registers; the prologue's register-held activation does not fit them.)  Measured, it stays VALU-bound well below the converted plan's
// rate: profiles/kquant_native.md.
#pragma once
#include "../../include/gpullama3_hip.h"
#include "gl3_decode_kernels.h"

namespace gl3 {

// v_pk_mul_f32 / v_pk_add_f32 are not wanted in these kernels (two f32 steps of one block in one instruction): scalar f32 only
#ifdef __HIP_DEVICE_COMPILE__
#define GL3_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define GL3_NO_PK_F32
#endif

constexpr int KQ_Q4K_TILE = 1216, KQ_Q5K_TILE = 1488, KQ_Q6K_TILE = 1792;
constexpr int KQ_NPW = 12;                    // producer wavefronts
// tiles per matrix a producer has in flight (two tiles either way: a SwiGLU launch streams two matrices), and the tile groups the
// producers finish as one batch = one chain segment: 24 groups (3072 elements), 12 (1536) for gate/up
__host__ __device__ constexpr int kq_ch(int epi) { return epi == EPI_SWIGLU ? 1 : 2; }
__host__ __device__ constexpr int kq_seg_groups(int epi) { return KQ_NPW * kq_ch(epi); }
constexpr int KQ_THREADS = 64 * (KQ_NPW + MV_AUX);
__host__ __device__ constexpr int kq_tile_bytes(int fmt) {
    return fmt == GL3_TYPE_Q4_K ? KQ_Q4K_TILE : fmt == GL3_TYPE_Q5_K ? KQ_Q5K_TILE : fmt == GL3_TYPE_Q6_K ? KQ_Q6K_TILE : TILE_BYTES;
}
// GGUF bytes of one super-block (256 elements) of a native format
__host__ __device__ constexpr int kq_superblock_bytes(int fmt) { return fmt == GL3_TYPE_Q4_K ? 144 : fmt == GL3_TYPE_Q5_K ? 176 : 210; }

// Row segments of one launch's matrices: the fused qkv matrix is built from up to three uploads of different formats (Q4_K_M:
// Q4_K, Q4_K, Q6_K; Q5_K_M: Q5_K, Q5_K, Q6_K).  seg[i] covers the strips from first_strip up to the next segment's; unused entries have
// first_strip = INT_MAX.
// seg2 = the second matrix of a SwiGLU pair (one segment; its format may differ from the first matrix's).
struct KqSeg { const uint8_t* base; int first_strip; int fmt; };
struct KqRec { KqSeg seg[3]; KqSeg seg2; };
// The SEL form's record (Qwen2-MoE, GL3_FLAG_KQUANT_NATIVE_MOE; one per MoeSlots record, a.kq points at it): the stacked tensors of the
// routed experts (exp / exp2 = gate / up, or down alone) and the shared expert's dense gate / up (sh / sh2), each ONE segment in its own
// format — four formats may meet in one launch.  Unit u of a matrix (expert sel[slot], or chunk slot - n_sel of the shared expert) starts
// u * (rows / 16) strips into its segment: byte offset u * (rows / 16) * ng * kq_tile_bytes(fmt).  first_strip is unused (0).
struct KqSelRec { KqSeg exp, exp2, sh, sh2; };

// what a producer lane holds of one (row, block) slot, whatever the format, and the Q8_0 block rebuilt from it
typedef int kq4i __attribute__((ext_vector_type(4)));
typedef int kq2i __attribute__((ext_vector_type(2)));
// Q8T: a / b = quants 0..15 / 16..31; Q4_K: a = nibbles; Q5_K: a = nibbles, b.x = fifth bits; Q6_K: a = low nibbles, b.xy = high bits
struct KqRaw { kq4i a, b; uint32_t h0, h1; };
struct KqBlock { kq4i lo, hi; float ws; };        // int8 quants 0..15 / 16..31, f16 scale widened

__device__ __forceinline__ const uint8_t* kq_uniform(const uint8_t* p) {      // a pointer every lane holds alike, into scalar registers
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<const uint8_t*>(((uint64_t)hi << 32) | lo);
}
template <typename T>
__device__ __forceinline__ T kq_ldnt(const uint8_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const T*>(p)); }

__device__ __forceinline__ KqRaw kq_load(int fmt, const uint8_t* p, int lane) {
    KqRaw r;
    r.b = (kq4i){0, 0, 0, 0}; r.h1 = 0;
    if (fmt == GL3_TYPE_Q4_K) {
        r.h1 = kq_ldnt<uint32_t>(p + 4 * (lane & 15));
        r.h0 = kq_ldnt<uint16_t>(p + 64 + 2 * lane);
        r.a = kq_ldnt<kq4i>(p + 192 + 16 * lane);
    } else if (fmt == GL3_TYPE_Q5_K) {
        r.h1 = kq_ldnt<uint32_t>(p + 4 * (lane & 15));
        const uint32_t top = kq_ldnt<uint8_t>(p + 64 + (lane & 15));
        r.h0 = kq_ldnt<uint16_t>(p + 80 + 2 * lane) | (((top >> (lane >> 4)) & 1) << 16);      // qarg whole again: bits 12..16
        r.b.x = (int)kq_ldnt<uint32_t>(p + 208 + 4 * lane);
        r.a = kq_ldnt<kq4i>(p + 464 + 16 * lane);
    } else if (fmt == GL3_TYPE_Q6_K) {
        r.h0 = kq_ldnt<uint32_t>(p + 4 * lane);
        const kq2i h = kq_ldnt<kq2i>(p + 256 + 8 * lane);
        r.b.x = h.x; r.b.y = h.y;
        r.a = kq_ldnt<kq4i>(p + 768 + 16 * lane);
    } else {                                    // Q8T (gl3_decode_kernels.h)
        r.h0 = kq_ldnt<uint16_t>(p + 2 * lane);
        r.a = kq_ldnt<kq4i>(p + 128 + 16 * lane);
        r.b = kq_ldnt<kq4i>(p + 1152 + 16 * lane);
    }
    return r;
}

// clamp(floor((double)p + 0.5), -128, 127) = Math.round(float) without the double: r = floor(p) and p - r decide.  p - r is exact
// except for p in (-0.5, 0), where it rounds inside [0.5, 1] and the answer (0) is the same.
__device__ __forceinline__ int kq_round_clamp(float p) {
    const float r = floorf(p);
    const int q = (int)r + ((p - r) >= 0.5f ? 1 : 0);
    return min(max(q, -128), 127);
}

// four nibbles (one per byte of n) -> the four int8 codes tab[nibble]
__device__ __forceinline__ uint32_t kq_map16(uint32_t n, const uint32_t (&tab)[4]) {
    const uint32_t sel = n & 0x07070707u;
    const uint32_t a = __builtin_amdgcn_perm(tab[1], tab[0], sel), b = __builtin_amdgcn_perm(tab[3], tab[2], sel);
    const uint32_t m = ((n >> 3) & 0x01010101u) * 0xFFu;
    return (b & m) | (a & ~m);
}

// Q4_KFloatTensor.getFloat: (d * sc) * q - dmin * m, left to right in f32
__device__ __forceinline__ float kq_q4k_value(float a, float b, int q) { return a * (float)q - b; }

__device__ __forceinline__ KqBlock kq_rebuild_q4k(const kq4i qs, uint32_t hdr, uint32_t ddm) {
    const float d = h2f((uint16_t)(ddm & 0xFFFF)), dmin = h2f((uint16_t)(ddm >> 16));
    const float a = d * (float)(hdr & 63), b = dmin * (float)((hdr >> 6) & 63);
    const float max_abs = fabsf(kq_q4k_value(a, b, (hdr >> 12) & 15));
    const float scale = max_abs / 127.0f;
    const float inv = scale != 0.f ? 1.0f / scale : 0.f;
    uint32_t tab[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) t |= (uint32_t)(kq_round_clamp(kq_q4k_value(a, b, 4 * j + i) * inv) & 0xFF) << (8 * i);
        tab[j] = t;
    }
    const uint32_t w[4] = {(uint32_t)qs.x, (uint32_t)qs.y, (uint32_t)qs.z, (uint32_t)qs.w};
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[2 * j] = kq_map16(w[j] & 0x0F0F0F0Fu, tab);
        o[2 * j + 1] = kq_map16((w[j] >> 4) & 0x0F0F0F0Fu, tab);
    }
    KqBlock r;
    r.lo = (kq4i){(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
    r.hi = (kq4i){(int)o[4], (int)o[5], (int)o[6], (int)o[7]};
    r.ws = (float)(_Float16)scale;
    return r;
}

// Q5_KFloatTensor.getFloat: Q4_K's value with q = nibble + 16 * fifth bit.  No table: each of the 32 elements is computed once.
__device__ __forceinline__ KqBlock kq_rebuild_q5k(const kq4i qs, uint32_t qh, uint32_t hdr, uint32_t ddm) {
    const float d = h2f((uint16_t)(ddm & 0xFFFF)), dmin = h2f((uint16_t)(ddm >> 16));
    const float a = d * (float)(hdr & 63), b = dmin * (float)((hdr >> 6) & 63);
    const float max_abs = fabsf(kq_q4k_value(a, b, (hdr >> 12) & 31));
    const float scale = max_abs / 127.0f;
    const float inv = scale != 0.f ? 1.0f / scale : 0.f;
    const uint32_t w[4] = {(uint32_t)qs.x, (uint32_t)qs.y, (uint32_t)qs.z, (uint32_t)qs.w};
    uint32_t o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t v = ((w[k >> 1] >> (4 * (k & 1))) & 0x0F0F0F0Fu) | (((qh >> k) & 0x01010101u) << 4);      // elements 4k .. 4k + 3
        uint32_t c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = (uint32_t)kq_round_clamp(kq_q4k_value(a, b, (v >> (8 * i)) & 0xFF) * inv);
        // the low bytes of the four clamped codes into one word: two v_perm_b32 (selector 0x0c = a zero byte) and an or
        o[k] = __builtin_amdgcn_perm(c[1], c[0], 0x0c0c0400u) | __builtin_amdgcn_perm(c[3], c[2], 0x04000c0cu);
    }
    KqBlock r;
    r.lo = (kq4i){(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
    r.hi = (kq4i){(int)o[4], (int)o[5], (int)o[6], (int)o[7]};
    r.ws = (float)(_Float16)scale;
    return r;
}

// Q6_KFloatTensor.getFloat: (d * sc) * (q - 32); v = four 6-bit values, one per byte
__device__ __forceinline__ float kq_q6k_value(float a, uint32_t v, int i) { return a * ((float)((v >> (8 * i)) & 0xFF) - 32.0f); }

__device__ __forceinline__ KqBlock kq_rebuild_q6k(const kq4i ql, const kq4i qh, uint32_t hdr) {
    const float d = h2f((uint16_t)(hdr >> 16));
    const float a0 = d * (float)(int8_t)(hdr & 0xFF), a1 = d * (float)(int8_t)((hdr >> 8) & 0xFF);
    const uint32_t w[4] = {(uint32_t)ql.x, (uint32_t)ql.y, (uint32_t)ql.z, (uint32_t)ql.w}, h[2] = {(uint32_t)qh.x, (uint32_t)qh.y};
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        v[k] = ((w[k >> 1] >> (4 * (k & 1))) & 0x0F0F0F0Fu) | (((h[k >> 2] >> (2 * (k & 3))) & 0x03030303u) << 4);
    float max_abs = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) max_abs = fmaxf(max_abs, fabsf(kq_q6k_value(k < 4 ? a0 : a1, v[k], i)));
    const float scale = max_abs / 127.0f;
    const float inv = scale != 0.f ? 1.0f / scale : 0.f;
    uint32_t o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) t |= (uint32_t)(kq_round_clamp(kq_q6k_value(k < 4 ? a0 : a1, v[k], i) * inv) & 0xFF) << (8 * i);
        o[k] = t;
    }
    KqBlock r;
    r.lo = (kq4i){(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
    r.hi = (kq4i){(int)o[4], (int)o[5], (int)o[6], (int)o[7]};
    r.ws = (float)(_Float16)scale;
    return r;
}

// the one device function every consumer of a native matrix goes through: matvec producers, embedding gather, gl3_debug_kquant_requant
__device__ __forceinline__ KqBlock kq_rebuild(int fmt, const KqRaw& r) {
    if (fmt == GL3_TYPE_Q4_K) return kq_rebuild_q4k(r.a, r.h0, r.h1);
    if (fmt == GL3_TYPE_Q5_K) return kq_rebuild_q5k(r.a, (uint32_t)r.b.x, r.h0, r.h1);
    if (fmt == GL3_TYPE_Q6_K) return kq_rebuild_q6k(r.a, r.b, r.h0);
    KqBlock q;
    q.lo = r.a; q.hi = r.b; q.ws = h2f((uint16_t)r.h0);
    return q;
}

// ---------------------------------------------------------------------------------------------------
// Decode matvec over native row segments: the structure of matvec_q8t_kernel (producers | aux prologue | chain wavefront, same LDS
// layout, same prologue and chain code, so the same sums in the same order) with KQ_NPW producers that rebuild every block before the
// dot.  The format is a wave-uniform value per strip (KqRec), so a fused qkv matrix of Q4_K / Q5_K and Q6_K segments, a SwiGLU pair of two
// formats and Q8T segments beside native ones (a Q8_0 tensor of the same file) all run in this one launch.
// SEGS: as in matvec_q8t_kernel, for strips of more than kq_seg_groups tile groups (K > 3072; gate/up: K > 1536).
// SEL: the routed experts of a Qwen2-MoE layer, blockIdx.y = slot, as matvec_q8t_kernel<.., SEL> (MoeSlots: x / out per slot, the shared
// expert's chunks as slots >= n_sel with a ragged last chunk).  The slot's one segment per matrix comes from the launch's KqSelRec and,
// for a routed slot, the expert id the router wrote: a scalar base and a scalar format per workgroup, so the producers below run the
// loads and rebuilds they run for a dense matrix.
template <int PRO, int EPI, bool SEGS, bool SEL = false>
__global__ GL3_NO_PK_F32 __launch_bounds__(KQ_THREADS, 4) void matvec_kq_kernel(const MatvecArgs a_in) {
    MatvecArgs a = a_in;
    int sel_fmt[2] = {0, 0};
    const uint8_t* sel_base[2] = {nullptr, nullptr};
    if (SEL) {
        const int slot = blockIdx.y;
        const MoeSlots m = *a.moe;
        const KqSelRec* ks = reinterpret_cast<const KqSelRec*>(a.kq);
        const bool routed = slot < m.n_sel;
        const int unit = __builtin_amdgcn_readfirstlane(routed ? m.sel[slot] : slot - m.n_sel);
        const size_t tiles = (size_t)unit * (a.rows / 16) * a.ng;
#pragma unroll
        for (int i = 0; i < (EPI == EPI_SWIGLU ? 2 : 1); ++i) {
            const KqSeg* sg = routed ? (i ? &ks->exp2 : &ks->exp) : (i ? &ks->sh2 : &ks->sh);
            sel_fmt[i] = __builtin_amdgcn_readfirstlane(sg->fmt);
            sel_base[i] = kq_uniform(sg->base) + tiles * kq_tile_bytes(sel_fmt[i]);
        }
        if (routed) {
            a.x += (size_t)slot * m.x_slot_stride;
            a.out += (size_t)slot * m.out_slot_stride;
        } else {
            a.out = m.sh_out + (size_t)unit * a.rows;
            const int left = m.sh_rows - unit * a.rows;
            if (left < a.rows) { a.rows = left; a.nstrips = (left + 15) / 16; }
        }
    }
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int NM = (EPI == EPI_SWIGLU) ? 2 : 1;
    constexpr int CH = kq_ch(EPI), NPW = KQ_NPW, SEG = kq_seg_groups(EPI);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nb4 = a.ng * 4;
    const int nbatch = SEGS ? ((a.ng + NPW - 1) / NPW + CH - 1) / CH : 1;
    uint8_t* xq = smem;
    float* xs = reinterpret_cast<float*>(smem + (size_t)nb4 * 32);
    float* xf = xs + nb4;
    float* pbuf = xf + (PRO == PRO_RMS ? a.k + 32 : 0);
    float* red = pbuf + (size_t)2 * NM * a.ng * 64;
    int* sync_w = reinterpret_cast<int*>(red + 4);
    if (t < 2) sync_w[t] = 0;

    if (wave < NPW) {
        // ------------------------------------------------------------------ producers
        // the row segments: read through the pointer and made scalar (the format decides wave-uniform branches)
        const KqRec* kr = a.kq;
        const int first1 = SEL ? INT32_MAX : __builtin_amdgcn_readfirstlane(kr->seg[1].first_strip);
        const int first2 = SEL ? INT32_MAX : __builtin_amdgcn_readfirstlane(kr->seg[2].first_strip);
        const int fmt1 = NM != 2 ? 0 : SEL ? sel_fmt[1] : __builtin_amdgcn_readfirstlane(kr->seg2.fmt);
        const uint8_t* base1 = NM != 2 ? nullptr : SEL ? sel_base[1] : kq_uniform(kr->seg2.base);
        const int nt = (a.ng - wave + NPW - 1) / NPW;
        KqRaw raw[NM][CH];
        int fmt0 = 0;
        auto issue = [&](int strip, int i0) __attribute__((always_inline)) {
            const KqSeg* sg = kr->seg + (strip >= first2 ? 2 : strip >= first1 ? 1 : 0);
            const uint8_t* sbase = SEL ? sel_base[0] : kq_uniform(sg->base);
            const int sfirst = SEL ? 0 : __builtin_amdgcn_readfirstlane(sg->first_strip);
            fmt0 = SEL ? sel_fmt[0] : __builtin_amdgcn_readfirstlane(sg->fmt);
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                if (i0 + u < nt) {
                    const int g = wave + (i0 + u) * NPW;
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const int fmt = m == 0 ? fmt0 : fmt1;
                        const size_t tile = (size_t)(m == 0 ? strip - sfirst : strip) * a.ng + g;
                        raw[m][u] = kq_load(fmt, (m == 0 ? sbase : base1) + tile * kq_tile_bytes(fmt), lane);
                    }
                }
            }
        };
        auto compute = [&](int i0, float* pb) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                if (i0 + u < nt) {
                    const int g = wave + (i0 + u) * NPW;
                    const int xb = 4 * g + (lane >> 4);
                    const int4 xlo = *reinterpret_cast<const int4*>(xq + 32 * xb);
                    const int4 xhi = *reinterpret_cast<const int4*>(xq + 32 * xb + 16);
                    const float xsc = xs[xb];
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const KqBlock q = kq_rebuild(m == 0 ? fmt0 : fmt1, raw[m][u]);
                        const int isum = dot32(q.lo, q.hi, xlo, xhi);
                        pb[(size_t)m * a.ng * 64 + g * 64 + lane] = (float)isum * (q.ws * xsc);
                    }
                }
            }
        };
        int strip = blockIdx.x;
        wg_barrier();
        if (strip < a.nstrips) issue(strip, 0);                  // HBM latency hides the activation prologue
        while (__hip_atomic_load(&sync_w[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) __builtin_amdgcn_s_sleep(2);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        int it = 0;
        for (; strip < a.nstrips; strip += gridDim.x, ++it) {
            float* pb = pbuf + (size_t)(it & 1) * NM * a.ng * 64;
            for (int i0 = 0; i0 < nt; i0 += CH) {
                if (it != 0 || i0 != 0) issue(strip, i0);
                compute(i0, pb);
                if (SEGS) lds_barrier();
            }
            if (SEGS) {
                for (int b = (nt + CH - 1) / CH; b < nbatch; ++b) lds_barrier();
            } else {
                wg_barrier();
            }
        }
        return;
    }

    // ---------------------------------------------------------------------- aux waves: the prologue of matvec_q8t_kernel
    __builtin_amdgcn_s_setprio(3);
    const int ta = t - 64 * NPW;
    const int nquads = a.k >> 2;
    float scale = 1.0f;
    constexpr int NXV = (PRO == PRO_RMS) ? 5 : 14;
    float4 nwv[5], xv[NXV];
#pragma unroll
    for (int i = 0; i < NXV; ++i) xv[i] = *reinterpret_cast<const float4*>(a.x + 4 * min(ta + 256 * i, nquads - 1));
    if (PRO == PRO_RMS) {
#pragma unroll
        for (int i = 0; i < 5; ++i) nwv[i] = *reinterpret_cast<const float4*>(a.norm_w + 4 * min(ta + 256 * i, nquads - 1));
    }
    wg_barrier();
    SubBarrier aux_sync{&sync_w[0], MV_AUX, 0};
    for (int b = (a.k >> 5) + ta; b < nb4; b += 256) {
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
        float ss;
        static_assert(ss_scratch_bytes(1000) == 128 + 3000, "the line below spells ss_scratch_bytes out (a call from here is not inlined, see wg_barrier; through an always_inline copy the listing changes)");
        if ((size_t)2 * NM * a.ng * 64 * 4 >= 128 + (size_t)3 * a.k && a.k >= 1024 && a.k <= 5120) {
            ss = exact_sumsq_lds(xf, a.k, reinterpret_cast<uint8_t*>(pbuf), ta, aux_sync);
        } else {
            if (wave == NPW) {
                const float s1 = seq_sum_lds<true>(xf, a.k);
                if (lane == 0) red[0] = s1;
            }
            aux_sync();
            ss = red[0];
        }
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
    aux_sync();
    if (ta == 0) __hip_atomic_store(&sync_w[1], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (wave != NPW) return;

    // ---------------------------------------------------------------------- chain wavefront: result += p_b, b ascending
    int it = 0;
    for (int strip = blockIdx.x; strip < a.nstrips; strip += gridDim.x, ++it) {
        const float* pb = pbuf + (size_t)(it & 1) * NM * a.ng * 64;
        v4f acc[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[m] = (v4f){0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < nbatch; ++b) {
            if (SEGS) lds_barrier(); else wg_barrier();
            int g = b * SEG;
            const int ge = SEGS ? min(g + SEG, a.ng) : a.ng;
            for (; g + 8 <= ge; g += 8) {
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
        if ((lane & 15) < 4) {
            const int r = lane & 3;
            const int row = strip * 16 + 4 * (lane >> 4) + r;
            if (row < a.rows) {
                const float v0 = r == 0 ? acc[0][0] : r == 1 ? acc[0][1] : r == 2 ? acc[0][2] : acc[0][3];
                float res;
                if (EPI == EPI_STORE) res = v0 * a.out_scale;
                if (EPI == EPI_RESID) res = a.resid_in ? a.resid_in[row] + v0 * a.out_scale : v0 * a.out_scale;
                if (EPI == EPI_SWIGLU) {
                    const float v1 = r == 0 ? acc[NM - 1][0] : r == 1 ? acc[NM - 1][1] : r == 2 ? acc[NM - 1][2] : acc[NM - 1][3];
                    const float gte = v0 / (float)(1.0 + exp(-(double)v0));
                    res = gte * v1;
                }
                a.out[row] = res;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Embedding row of a native token_embd: x[i] = ((float)q8[i] * d8) * emb_scale of the rebuilt blocks — what embed_q8t_kernel reads
// from the converted matrix.  One thread per 32-block of the row.
static __global__ GL3_NO_PK_F32 __launch_bounds__(256) void embed_kq_kernel(const uint8_t* __restrict__ emb, int fmt, int ng, int dim,
                                                                      const int* __restrict__ dyn, float* __restrict__ x, float emb_scale) {
    const int token = dyn[0];
    const uint8_t* strip = emb + (size_t)(token >> 4) * ng * kq_tile_bytes(fmt);
    for (int b = threadIdx.x; b < (dim >> 5); b += 256) {
        const KqBlock q = kq_rebuild(fmt, kq_load(fmt, strip + (size_t)(b >> 2) * kq_tile_bytes(fmt), (token & 15) + 16 * (b & 3)));
        const int w[8] = {q.lo.x, q.lo.y, q.lo.z, q.lo.w, q.hi.x, q.hi.y, q.hi.z, q.hi.w};
#pragma unroll
        for (int e = 0; e < 32; ++e) x[32 * b + e] = ((float)(int8_t)(w[e >> 2] >> (8 * (e & 3))) * q.ws) * emb_scale;
    }
}

// gl3_debug_kquant_requant: the rebuilt block of every (row, block) slot as a GGUF Q8_0 block (f16 d | 32 x int8)
static __global__ GL3_NO_PK_F32 __launch_bounds__(256) void kq_requant_kernel(const uint8_t* __restrict__ tiles, int fmt, int rows, int nb, int ng,
                                                                        uint8_t* __restrict__ dst) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)rows * nb) return;
    const int row = (int)(idx / nb), b = (int)(idx % nb);
    const KqBlock q = kq_rebuild(fmt, kq_load(fmt, tiles + ((size_t)(row >> 4) * ng + (b >> 2)) * kq_tile_bytes(fmt), (row & 15) + 16 * (b & 3)));
    uint16_t* o = reinterpret_cast<uint16_t*>(dst + (size_t)idx * 34);
    o[0] = __builtin_bit_cast(uint16_t, (_Float16)q.ws);
    const int w[8] = {q.lo.x, q.lo.y, q.lo.z, q.lo.w, q.hi.x, q.hi.y, q.hi.z, q.hi.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) o[1 + i] = (uint16_t)((uint32_t)w[i >> 1] >> (16 * (i & 1)));
}

// ---------------------------------------------------------------------------------------------------
// Repack at upload: GGUF super-blocks (256 elements) of `rows` rows of nb 32-blocks -> the tiles above, one thread per destination
// (row, block) slot, rows padded to 16 with zero slots (d = 0: every code and the scale are 0).
// Q4_K super-block (144 B): f16 d | f16 dmin | 12 B packed 6-bit scales / mins | 128 nibble bytes; sub-block j = 2p (low nibbles of
// bytes 32p .. 32p + 31) or 2p + 1 (their high nibbles).
static __global__ GL3_NO_PK_F32 void repack_q4k_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int nb, int ng) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int rows16 = (rows + 15) & ~15;
    if (idx >= (long)rows16 * nb) return;
    const int row = (int)(idx / nb), pb = (int)(idx % nb);
    uint8_t* tile = dst + ((size_t)(row >> 4) * ng + (pb >> 2)) * KQ_Q4K_TILE;
    const int l = (row & 15) + 16 * (pb & 3);
    uint32_t ddm = 0, hdr = 0, w[4] = {0, 0, 0, 0};
    if (row < rows) {
        const uint8_t* sb = src + ((size_t)row * (nb >> 3) + (pb >> 3)) * 144;
        const int j = pb & 7;
        ddm = (uint32_t)sb[0] | ((uint32_t)sb[1] << 8) | ((uint32_t)sb[2] << 16) | ((uint32_t)sb[3] << 24);
        const uint8_t* sc = sb + 4;
        const int s = j < 4 ? (sc[j] & 63) : ((sc[j + 4] & 0xF) | ((sc[j - 4] >> 6) << 4));          // Q4_KFloatTensor.getScaleK4 / getMinK4
        const int m = j < 4 ? (sc[j + 4] & 63) : ((sc[j + 4] >> 4) | ((sc[j] >> 6) << 4));
        const uint8_t* qs = sb + 16 + (j >> 1) * 32;
        int qmin = 15, qmax = 0;
        for (int e = 0; e < 32; ++e) {
            const int q = (j & 1) ? (qs[e] >> 4) : (qs[e] & 0xF);
            qmin = min(qmin, q); qmax = max(qmax, q);
            w[e >> 3] |= (uint32_t)q << (8 * (e & 3) + 4 * ((e >> 2) & 1));
        }
        const float a = h2f((uint16_t)(ddm & 0xFFFF)) * (float)s, b = h2f((uint16_t)(ddm >> 16)) * (float)m;
        const int qarg = fabsf(kq_q4k_value(a, b, qmax)) >= fabsf(kq_q4k_value(a, b, qmin)) ? qmax : qmin;
        hdr = (uint32_t)s | ((uint32_t)m << 6) | ((uint32_t)qarg << 12);
    }
    if ((pb & 3) == 0) *reinterpret_cast<uint32_t*>(tile + 4 * (row & 15)) = ddm;
    *reinterpret_cast<uint16_t*>(tile + 64 + 2 * l) = (uint16_t)hdr;
    *reinterpret_cast<uint4*>(tile + 192 + 16 * l) = make_uint4(w[0], w[1], w[2], w[3]);
}

// Q5_K super-block (176 B): f16 d | f16 dmin | 12 B scales / mins as Q4_K | 32 fifth-bit bytes | 128 nibble bytes; the fifth bit of
// element e of sub-block j is bit j of byte e.  One thread per destination (row, tile) = the four slots that share the row's u8 of
// qarg top bits.
static __global__ GL3_NO_PK_F32 void repack_q5k_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int nb, int ng) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int rows16 = (rows + 15) & ~15;
    if (idx >= (long)rows16 * ng) return;
    const int row = (int)(idx / ng), g = (int)(idx % ng);
    uint8_t* tile = dst + ((size_t)(row >> 4) * ng + g) * KQ_Q5K_TILE;
    uint32_t ddm = 0, top = 0;
    for (int c = 0; c < 4; ++c) {
        const int pb = 4 * g + c, l = (row & 15) + 16 * c;
        uint32_t hdr = 0, h = 0, w[4] = {0, 0, 0, 0};
        if (row < rows) {
            const uint8_t* sb = src + ((size_t)row * (nb >> 3) + (pb >> 3)) * 176;
            const int j = pb & 7;
            ddm = (uint32_t)sb[0] | ((uint32_t)sb[1] << 8) | ((uint32_t)sb[2] << 16) | ((uint32_t)sb[3] << 24);
            const uint8_t* sc = sb + 4;
            const int s = j < 4 ? (sc[j] & 63) : ((sc[j + 4] & 0xF) | ((sc[j - 4] >> 6) << 4));          // Q4_KFloatTensor.getScaleK4 / getMinK4
            const int m = j < 4 ? (sc[j + 4] & 63) : ((sc[j + 4] >> 4) | ((sc[j] >> 6) << 4));
            const uint8_t* qh = sb + 16;
            const uint8_t* qs = sb + 48 + (j >> 1) * 32;
            int qmin = 31, qmax = 0;
            for (int e = 0; e < 32; ++e) {
                const uint32_t lo = (j & 1) ? (qs[e] >> 4) : (qs[e] & 0xF), hi = (qh[e] >> j) & 1;
                const int q = (int)(lo | (hi << 4));
                qmin = min(qmin, q); qmax = max(qmax, q);
                w[e >> 3] |= lo << (8 * (e & 3) + 4 * ((e >> 2) & 1));
                h |= hi << (8 * (e & 3) + (e >> 2));
            }
            const float a = h2f((uint16_t)(ddm & 0xFFFF)) * (float)s, b = h2f((uint16_t)(ddm >> 16)) * (float)m;
            const int qarg = fabsf(kq_q4k_value(a, b, qmax)) >= fabsf(kq_q4k_value(a, b, qmin)) ? qmax : qmin;
            hdr = (uint32_t)s | ((uint32_t)m << 6) | ((uint32_t)(qarg & 15) << 12);
            top |= (uint32_t)(qarg >> 4) << c;
        }
        *reinterpret_cast<uint16_t*>(tile + 80 + 2 * l) = (uint16_t)hdr;
        *reinterpret_cast<uint32_t*>(tile + 208 + 4 * l) = h;
        *reinterpret_cast<uint4*>(tile + 464 + 16 * l) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint32_t*>(tile + 4 * (row & 15)) = ddm;
    tile[64 + (row & 15)] = (uint8_t)top;
}

// Q6_K super-block (210 B): 128 low-nibble bytes | 64 high-2-bit bytes | 16 int8 scales | f16 d.  Block j = 4 * half + grp: element e has
// its low nibble in ql[64 half + 32 (grp & 1) + e] (>> 4 for grp >= 2), its high bits in qh[32 half + e] >> 2 grp, scale 8 half + 2 grp + e / 16.
static __global__ GL3_NO_PK_F32 void repack_q6k_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int nb, int ng) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int rows16 = (rows + 15) & ~15;
    if (idx >= (long)rows16 * nb) return;
    const int row = (int)(idx / nb), pb = (int)(idx % nb);
    uint8_t* tile = dst + ((size_t)(row >> 4) * ng + (pb >> 2)) * KQ_Q6K_TILE;
    const int l = (row & 15) + 16 * (pb & 3);
    uint32_t hdr = 0, w[4] = {0, 0, 0, 0}, h[2] = {0, 0};
    if (row < rows) {
        const uint8_t* sb = src + ((size_t)row * (nb >> 3) + (pb >> 3)) * 210;
        const int j = pb & 7, half = j >> 2, grp = j & 3;
        const uint8_t* ql = sb + 64 * half + 32 * (grp & 1);
        const uint8_t* qh = sb + 128 + 32 * half;
        for (int e = 0; e < 32; ++e) {
            const uint32_t lo = (ql[e] >> (4 * (grp >> 1))) & 0xF, hi = (qh[e] >> (2 * grp)) & 3;
            w[e >> 3] |= lo << (8 * (e & 3) + 4 * ((e >> 2) & 1));
            h[e >> 4] |= hi << (8 * (e & 3) + 2 * ((e >> 2) & 3));
        }
        hdr = (uint32_t)sb[192 + 8 * half + 2 * grp] | ((uint32_t)sb[193 + 8 * half + 2 * grp] << 8) | ((uint32_t)sb[208] << 16) | ((uint32_t)sb[209] << 24);
    }
    *reinterpret_cast<uint32_t*>(tile + 4 * l) = hdr;
    *reinterpret_cast<uint2*>(tile + 256 + 8 * l) = make_uint2(h[0], h[1]);
    *reinterpret_cast<uint4*>(tile + 768 + 16 * l) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace gl3
