// gl3_kv_copy.h — gl3_kv_seq_copy: the K and V rows [p0, p1) of one sequence slot, every layer, copied to the same positions of other slots.
//
// The cache is f32 [n_seqs][L][ctx][kv_dim_l] (gl3_ctx.h), so within one layer the rows [p0, p1) of a sequence are ONE contiguous span of
// (p1 - p0) * kv_dim_l floats at (layer * ctx + p0) * kv_dim_l from the sequence's base: a call moves 2 * L spans (K, then V) and the kernel
// is a plain streaming copy over them, cut into chunks of KVC_CHUNK4 float4.  One launch does K and V, all layers and all destinations: a
// workgroup loads a chunk of the source span ONCE into registers and stores it to every destination, so the fan-out multiplies the bytes
// written, never the bytes read.
//
// Alignment: every access is a float4.  kv_dim_l = kv_heads_l * head_size is a multiple of 32 floats (gl3_create refuses other head sizes), so
// a row is a multiple of 128 bytes; hipMalloc returns 256-byte-aligned bases; kv_seq_stride, the layer stride and the span offset are whole rows.
// Every span therefore starts and ends on a 16-byte boundary (gl3_kv_seq_copy checks kv_dim_l % 4 before it launches).
// Offsets: everything that is scaled by a sequence, layer or position is size_t — a real plan's cache is larger than 2^32 bytes (8 slots x 32
// layers x 8192 rows x 1024 floats = 8 GiB per cache).  Only the chunk counter is 32-bit (2^32 chunks of 16 KiB = 64 TiB per call; checked).
//
// Shape of a workgroup's trip: 256 threads x KVC_UNROLL = 4 independent 16-byte loads per lane = 16 KiB per chunk in flight, then the stores.
// The kernel needs few registers, so a CU holds 8 such workgroups (its 32 wavefront slots): up to 128 KiB of loads in flight per CU, past the
// ~32 KiB per CU at which the HBM pipe streams.  The grid is sized from the bytes: one workgroup per chunk up to 8 per CU, grid-stride beyond —
// a 1-row copy launches 2 * L workgroups, a 4096-row one 2048.  A span is not a multiple of the chunk in general: the last chunk of a span
// guards every float4 (no read or write past the span), the others run unguarded.
//
// Stores are plain, not non-temporal: see the measurement note at KVC_NT_STORES.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace gl3 {

constexpr int KVC_THREADS = 256, KVC_UNROLL = 4, KVC_CHUNK4 = KVC_THREADS * KVC_UNROLL;      // float4 per chunk
constexpr int KVC_WGS_PER_CU = 8;
static_assert(KVC_CHUNK4 * 16 == 16 * 1024, "a chunk is 16 KiB");

// Plain or non-temporal stores, by measurement (scripts/kv_copy_bw.py on one MI355X, Llama-3-8B K / V shape, median of 30 calls, host clock around
// the call; the same process probes 4.8 - 4.9 TB/s for a device-to-device copy, bytes = read + written; plain was run twice, around the other):
//                                   plain stores               non-temporal stores (-DKVC_NT_STORES=1)
//    512 rows -> 1 slot   (256 MiB)   65 / 66 us   4.1 TB/s      57 us   4.7 TB/s
//    512 rows -> 7 slots  (1 GiB)    243 / 245 us  4.4 TB/s     201 us   5.3 TB/s
//   4096 rows -> 1 slot   (2 GiB)    427 / 425 us  5.0 TB/s     421 us   5.1 TB/s
//   4096 rows -> 7 slots  (8 GiB)   1748 / 1725 us 4.9 TB/s    1763 us   4.9 TB/s
//   the decode row at position 512 on the destination, right behind the 512-row copy:   2475 / 2487 us      2732 us   (at 4096: 10.9 ms both)
// Both forms run at the probed copy rate once the copy is large; non-temporal stores win 8 us (one slot) to 43 us (seven) on the 512-row copy,
// but the destination's rows are what the very next attention launch reads, and behind plain stores that step is ~250 us faster: 128 MiB of
// copied rows are still in the 256 MiB Infinity Cache.  The fork exists for that next step, so the stores are plain.  (Loads are plain either
// way: the source rows were just written, or are about to be read by their own sequence.)  A build with -DKVC_NT_STORES=1 is the other form;
// scripts/kv_copy_bw.py measures whichever library GL3_LIB names.
#ifndef KVC_NT_STORES
#define KVC_NT_STORES 0
#endif

typedef float kvc_v4f __attribute__((ext_vector_type(4)));

struct KvCopyArgs {
    float* kcache;
    float* vcache;
    int n_dst, src_seq, n_layers;
    size_t seq_stride4;           // float4 per sequence
    size_t layer_stride4;         // float4 per layer = ctx * kv_dim_l / 4
    size_t span_off4;             // p0 * kv_dim_l / 4
    size_t span4;                 // (p1 - p0) * kv_dim_l / 4
    uint32_t chunks_per_span;     // ceil(span4 / KVC_CHUNK4)
    uint32_t n_chunks;            // 2 * n_layers * chunks_per_span
};

template <bool GUARD>
static __device__ __forceinline__ void kvc_chunk(const KvCopyArgs& a, const int* __restrict__ dst_seqs, kvc_v4f* base, size_t i0) {
    const kvc_v4f* src = base + (size_t)a.src_seq * a.seq_stride4;
    kvc_v4f v[KVC_UNROLL];
#pragma unroll
    for (int u = 0; u < KVC_UNROLL; ++u)
        if (!GUARD || i0 + (size_t)u * KVC_THREADS < a.span4) v[u] = src[i0 + (size_t)u * KVC_THREADS];
    auto put = [&](int d) {
        kvc_v4f* dst = base + (size_t)dst_seqs[d] * a.seq_stride4;
#pragma unroll
        for (int u = 0; u < KVC_UNROLL; ++u)
            if (!GUARD || i0 + (size_t)u * KVC_THREADS < a.span4) {
#if KVC_NT_STORES
                __builtin_nontemporal_store(v[u], dst + i0 + (size_t)u * KVC_THREADS);
#else
                dst[i0 + (size_t)u * KVC_THREADS] = v[u];
#endif
            }
    };
    // the first destination outside the loop: the wait for the loads then sits in front of it, and the loop's trips, which read the same
    // registers with only stores outstanding, issue their stores without waiting for the previous destination's to drain
    put(0);
    for (int d = 1; d < a.n_dst; ++d) put(d);
}

// dst_seqs: n_dst distinct sequence ids in device memory, none of them src_seq.  A __restrict__ kernel argument of its own: the compiler then reads
// the ids with scalar loads, which the vector-memory counter does not see — as a plain pointer they are vector loads, and the wait for an id
// also waits for every store of the previous destination.
static __global__ __launch_bounds__(KVC_THREADS) void kv_seq_copy_kernel(KvCopyArgs a, const int* __restrict__ dst_seqs) {
    for (uint32_t c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const uint32_t span = c / a.chunks_per_span, within = c - span * a.chunks_per_span;      // spans 0 .. L-1: K of layer span; L .. 2L-1: V
        const bool is_v = span >= (uint32_t)a.n_layers;
        const size_t layer = is_v ? span - (uint32_t)a.n_layers : span;
        kvc_v4f* base = reinterpret_cast<kvc_v4f*>(is_v ? a.vcache : a.kcache) + layer * a.layer_stride4 + a.span_off4;
        const size_t i0 = (size_t)within * KVC_CHUNK4 + threadIdx.x;
        if ((size_t)(within + 1) * KVC_CHUNK4 <= a.span4) kvc_chunk<false>(a, dst_seqs, base, i0);
        else kvc_chunk<true>(a, dst_seqs, base, i0);
    }
}

}      // namespace gl3
