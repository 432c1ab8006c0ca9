// gl3_bd_gemm.h — the Q8_0 batched-matmul argument block and the small-batch GEMM (static-batched decode, prefill chunks of <= 64
// tokens).
// (Round 1's producer / chain-wavefront kernel, 32 rows x 32 tokens per workgroup with an LDS ring and a barrier per 8 blocks,
// is in the history: 106 us of GEMMs per Qwen3-4B layer at B = 32 against 53 us for the kernel below.)
// Included by gl3_prefill.hip (product) and by scripts/probes/bd_probe.hip (stand-alone timing harness), both after
// `using namespace gl3;`.
#pragma once
#include "gl3_decode_kernels.h"
#include <type_traits>

typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v16i_t __attribute__((ext_vector_type(16)));
typedef float v2f_t __attribute__((ext_vector_type(2)));
typedef long v2l_t __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------
// Batched Q8_0 matmul: out[b][n] = sum_blocks float(isum) * (wScale * aScale), blocks ascending
// (FloatTensor.matmul(context, ...) :102-111 with dotQ8Activation).
struct GemmArgs {
    const uint8_t* w; const uint8_t* w2;  // Q8T matrices (w2: up projection for the SwiGLU epilogue)
    int rows, ng, nb;                     // valid rows, tile groups per strip, real blocks per row (k/32)
    const uint8_t* XQ; const float* XS; int maxk;
    int tslots;                           // bdw_gemm_kernel: token slots of the XQ2 / XS2 layout (32 or 64); 0 = row layout
    int ntt, nrt;                         // token tiles, row tiles (grid = 8 * ceil(ntt * nrt / 8), see the XCD mapping)
    int ntok;
    float* out; int out_stride;           // EPI_STORE / EPI_SWIGLU: out[b*stride + row]; EPI_RESID: out +=
    float out_scale;                      // EPI_STORE / EPI_RESID: result *= out_scale first (Granite; 1 otherwise, exact)
    uint8_t* XQo; float* XSo;             // bdw_gemm_kernel<EPI_SWIGLU, .., QOUT>: hb leaves the kernel quantised (XQ2 / XS2 layout)
    uint8_t* XPo;                         // pf_gemm3t_kernel<.., QOUT>: the quantised hb's scale-operand table (XQo = its int8 chunks)
    const uint8_t* XP; int xp_tok;        // pf_gemm3_kernel: activation scale operands XP[block][half][xp_tok token slots][16 B] (gl3_prefill_gemm3.h)
    // bdw_gemm_kernel<.., GRP>: the routed experts of a Qwen2-MoE step (tile table and sorted slots: moe_group_kernel, gl3_moe_kernels.h)
    const int* gtab;                      // gtab[0] = entries; entry u = gtab[4 + 4u ..] = (expert, first sorted slot, valid slots <= 16)
    const int* gtok;                      // token slot of the operand per sorted slot (gate + up); null = the sorted slot itself (down)
    const int* gdst;                      // output row per sorted slot (down: token * (topk + 1) + choice); null = the sorted slot itself
    int gspe;                             // strips per expert (rows = rows of ONE expert; w / w2 = the stacked tensors)
};


// ---------------------------------------------------------------------------------------------------
// Static-batched decode and small prefill chunks, wave-owned form (<= 64 tokens).  One wavefront = one workgroup = 16 weight rows (one Q8T strip) x
// 16 tokens x ALL of K, result in registers, accumulated block by block in the reference's order.  No operand staging in LDS,
// no barriers; grid = strips x token tiles (the token tiles of a strip 8 workgroup ids apart: same XCD, one L2).
//   * one v_mfma_i32_16x16x32_i8 per (block, token tile).  The Q8T tile stores a block row as two 16-byte halves, so a
//     lane's natural load is 16 B: lane (row r, k-group g) loads half g & 1 of block 2j + (g >> 1) — two blocks per
//     load — and two v_permlane32_swap turn that into the 8 B x 4 k-groups of block 2j (low registers) and of block
//     2j + 1 (high registers).  The int8 dot is exact, so the order of k inside a block is free; only A and B have to
//     agree, and B (the int8 activations) is stored pre-split for exactly this access (XQ2 below): no swap on that side.
//   * weight scales: the 128-byte f16 header of TWO tiles per load (lanes 0-31 / 32-63), converted once and parked in LDS
//     as f32, read back as one broadcast float4 = the 4 rows a lane accumulates.  Activation scales: one float per lane
//     and tile, parked in LDS twice ({s, s} = a ready v_pk_mul operand).
//   * a tile runs in two halves one iteration apart — front(i + 1): swaps + MFMAs, back(i): (float)isum * (wScale * aScale)
//     and result += p, blocks ascending — so the MFMA latency sits behind the previous tile's arithmetic.
//   * addresses are a uniform base (SGPRs, advanced by scalar adds) + a loop-invariant per-lane offset, and NOTHING is
//     clamped or guarded: the rings read up to DA tiles past the end of a strip / of the activations, which is why
//     every weight matrix and XQ2 / XS2 carry GL3_TAIL_PAD bytes of slack (alloc_mat, gl3_prefill_init).  A load under a
//     condition makes the compiler wait vmcnt(0) at every use ("conditional loads"), and so did several other
//     constructs here — ring slots must not be float4s whose odd elements feed v_pk_mul broadcasts, a later tile's swaps
//     must not be scheduled behind their loads (sched_barrier per tile), the prologue has to issue in the loop's order,
//     loop exits inside the unrolled trip split the ring's live ranges, and since vmcnt counts in issue order every stream
//     (weights from HBM, activations from L2) needs the same ring depth.
//   * SwiGLU: gate and up rows of a strip in one wavefront (NM = 2): the activations are fetched once for both matrices.
//     QOUT: a workgroup is the two strips of one 32-row block of hb and writes it quantised for the down projection
//     (block maximum through LDS in the epilogue) — one launch and one f32 round trip less per layer.
// Measured dead ends (scripts/probes/bd_probe.hip): k-slices per strip with an adding wavefront or an owning slice
// (LDS exchange + one barrier per round: never faster than one wavefront per strip, 17-22 us vs 17.7 on the 2560 x 9728
// matrix); token tiles of a strip in one workgroup; rings deeper than 8 tiles; non-temporal weight loads (the token tiles
// re-read the lines from L2); gate and up as separate wavefronts with silu(g) * u in the next quantiser (2432 single-matrix
// wavefronts fetch the activations twice: 21-22 us vs 18.3 fused).
// GRP (Qwen2-MoE routed experts): the same wavefront over a (tile-table entry, strip of the entry's expert) instead of a (token tile,
// strip).  The 16 tokens of an entry are 16 sorted (token, choice) slots of one expert; lane t's operand address is its own token's
// (gtok[slot] * 64 + 16 g instead of (16 h + t) * 64 + 16 g: the gather is one index load per lane, no copy), the token-slot count of
// XQ2 / XS2 is the run-time a.tslots (any chunk length; advancing stays a scalar add), lanes past the entry's valid count point at its
// last valid slot and store nothing, and the result rows go to gdst[slot] (the scatter of the down projection).  Workgroups past the
// table's entry count exit: the grid is sized for the bound moe_group_max_entries() from the step's token count alone.
// Placement: workgroup id = entry * gspe + strip, so the entries of one expert that stream the same strip sit gspe ids apart.  With gspe a
// multiple of 8 (88 and 128 strips at the A2.7B shape) they share id % 8, i.e. the XCD and its L2, as the token tiles of a dense strip
// do (bdw_grid); for another gspe the rule is not kept and an expert with several entries re-reads its strips through several L2s
// (not measured).  An odd number
// of tiles per strip (K = 1408: 11, K = 384: 3, K = 128: 1) needs nothing special: the header load of the last, even-numbered tile
// also fetches the header of the tile behind the strip (slack, or the next strip), whose scales are parked and never read.
// Activation layout (written by pf_norm_quant_kernel when tslots != 0), tslots = 32 or 64 token slots (template parameter TS):
//   XS2[k / 128][tslots][4] f32 = the 4 block scales of a tile;
//   XQ2[k / 64][tslots][64] int8 = blocks 2j, 2j + 1 of a token, already in the lanes' operand order: bytes 16g .. 16g + 7 =
//   k-chunk c(g) of block 2j, bytes 16g + 8 .. 16g + 15 = the same chunk of block 2j + 1, with c(0..3) = k 0-7, 16-23, 8-15,
//   24-31 (what the swap leaves in k-group g on the weight side) — bdq_offset() in gl3_decode_kernels.h.
constexpr int BD_TS = 32, BD_TS_MAX = 64;            // token slots: 32 (<= 32 tokens) or 64 (33 .. 64)

// grid: workgroup id -> (strip, token tile).  The token tiles of a strip stream the same weights, so they sit 8 ids apart: same
// XCD (= id % 8), i.e. one L2, and dispatched together.
__host__ __device__ inline int bdw_grid(int strips, int nt) { return ((strips + 7) / 8) * 8 * nt; }
// ... of a launch of ntg token tiles: the token tile and the unit (strip; QOUT: strip pair) of workgroup id
__host__ __device__ inline int bdw_place_tile(unsigned id, int ntg) { return (id >> 3) % ntg; }
__host__ __device__ inline int bdw_place_unit(unsigned id, int ntg) { return (id / (8 * ntg)) * 8 + (id & 7); }

// Token slots of the XQ / XS operand layout above when a step of n tokens runs on bdw_gemm_kernel (n <= 64), 0 for a larger step.
inline int bd_tslots(int n) { return n <= BD_TS ? BD_TS : n <= BD_TS_MAX ? BD_TS_MAX : 0; }

// The launch of one GEMM of a step of at most 64 tokens: what launch_gemm (gl3_prefill.hip) launches and, with no device, what
// gl3_debug_bd_gemm_plan answers.  epi: EPI_STORE / EPI_RESID (DA 8) or EPI_SWIGLU (DA 4; quantised_out: the two-strip form that writes hb
// as the down projection's operand).  tslots 0: more than 64 tokens, not this kernel (every other field 0).
struct BdGemmPlan {
    int tslots, DA, qout, threads;                   // TS, ring depth, the quantising form, threads per workgroup
    int ntt, units, grid;                            // token tiles, strips (qout: strip pairs), workgroups (units padded to 8, x ntt)
    int ntiles, trips, partial;                      // K: tiles of 4 blocks, full trips of DA tiles, tiles of the partial last trip (0: none)
};
inline BdGemmPlan bd_gemm_plan(int epi, int rows, int k, int ntok, bool quantised_out) {
    BdGemmPlan p{};
    p.tslots = bd_tslots(ntok);
    if (!p.tslots) return p;
    p.DA = epi == EPI_SWIGLU ? 4 : 8;
    p.qout = epi == EPI_SWIGLU && quantised_out;
    p.threads = p.qout ? 128 : 64;
    p.ntt = (ntok + 15) / 16;
    p.units = p.qout ? (rows + 31) / 32 : (rows + 15) / 16;
    p.grid = bdw_grid(p.units, p.ntt);
    const int nb = k / 32;
    p.ntiles = (nb + 3) / 4;
    p.trips = (nb >> 2) / p.DA;
    p.partial = p.ntiles - p.trips * p.DA;
    return p;
}

template <int EPI, int DA, int WPE, bool QOUT = false, int TS = BD_TS, bool GRP = false>
__global__ __launch_bounds__(QOUT ? 128 : 64, WPE) void bdw_gemm_kernel(const GemmArgs a) {
    static_assert(!QOUT || EPI == EPI_SWIGLU, "the quantising epilogue is the SwiGLU one");
    static_assert(!GRP || !QOUT, "the grouped form writes f32");
    constexpr int NWV = QOUT ? 2 : 1;                  // QOUT: two wavefronts = the two strips of one 32-row activation block
    constexpr int NM = (EPI == EPI_SWIGLU) ? 2 : 1;
    static_assert(DA % 2 == 0, "ring slots are static under the unroll");
    __shared__ __attribute__((aligned(16))) float wsl_all[NWV][4 * NM * 64];   // [tile & 3][matrix][block][row] weight scales
    __shared__ __attribute__((aligned(16))) float xsl_all[NWV][4 * 128];       // [tile & 3][blocks 01 | 23][token][2 blocks][2]: activation scale pairs, a token's float4s 16 B apart (no bank conflicts)
    __shared__ float amax_s[NWV][64];
    const int lane = threadIdx.x & 63, t = lane & 15, g = lane >> 4;
    const int wv = QOUT ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
#ifdef BDW_TIMING
    const unsigned long long bdw_t0 = __builtin_readcyclecounter(), bdw_w0 = wall_clock64();
#endif
    float* wsl = wsl_all[wv];
    float* xsl = xsl_all[wv];
    const int NTG = (a.ntok + 15) >> 4;                                         // token tiles of this launch
    const int nstrips = (a.rows + 15) >> 4;
    const int h = GRP ? 0 : bdw_place_tile(blockIdx.x, NTG);
    const int unit = GRP ? (int)(blockIdx.x % a.gspe) : bdw_place_unit(blockIdx.x, NTG);                   // strip (QOUT: strip pair; GRP: of the entry's expert)
    int strip = unit * NWV + wv;                                                // QOUT: rows % 32 == 0, so both strips exist
    int gfirst = 0, gcnt = 16, gslot = 0;                                       // GRP: the entry's sorted slots, this lane's slot
    uint32_t tokslot = 16 * h + t;                                              // this lane's token slot of XQ2 / XS2
    if constexpr (GRP) {
        const int u = blockIdx.x / a.gspe;
        if (u >= a.gtab[0]) return;                                             // the grid is sized for the bound on the table
        const int4 en = *reinterpret_cast<const int4*>(a.gtab + 4 + 4 * u);
        strip += en.x * a.gspe;
        gfirst = en.y; gcnt = en.z;
        gslot = gfirst + min(t, gcnt - 1);                                      // lanes past the ragged end: the last valid slot
        tokslot = a.gtok ? a.gtok[gslot] : gslot;
    } else if (unit * NWV >= nstrips) return;                                   // padding of the grid to a multiple of 8 units
    const int ts = GRP ? a.tslots : TS;                                         // token slots per block pair of XQ2 (GRP: run time)
    const int ntiles = a.ng;
    const size_t strip_bytes = (size_t)a.ng * TILE_BYTES;
    // uniform stream bases of the NEXT tile to fetch, advanced by scalar adds
    const uint8_t* pa[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) pa[m] = (m == 0 ? a.w : a.w2) + (size_t)strip * strip_bytes;
    const uint8_t* pb = a.XQ;
    const float* px = a.XS;
    const uint32_t la = ((g & 1) ? 1152 : 128) + 16 * (t + 16 * (g >> 1));       // + 512 for the tile's second block pair
    const uint32_t lh = (lane >> 5) * TILE_BYTES + 4 * (lane & 31);              // headers of tiles i (lanes 0-31), i + 1 (32-63)
    const uint32_t lb = tokslot * 64 + 16 * g;                                   // + ts * 64 for the second pair
    const uint32_t lx = (tokslot * 4 + g) * 4;
    v4i_t Ar[NM][DA][2]; uint32_t Hr[NM][DA / 2]; v2l_t Br[DA][2]; float Xr[DA];
    auto fetch = [&](int u) {                            // the tile at the stream heads -> ring slot u; heads advance one tile
#pragma unroll
        for (int m = 0; m < NM; ++m) {
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) Ar[m][u][jj] = *reinterpret_cast<const v4i_t*>(pa[m] + la + 512 * jj);
            if ((u & 1) == 0) Hr[m][u / 2] = *reinterpret_cast<const uint32_t*>(pa[m] + lh);
            pa[m] += TILE_BYTES;
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) Br[u][jj] = *reinterpret_cast<const v2l_t*>(pb + lb + jj * (ts * 64));
        Xr[u] = *reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(px) + lx);
        pb += 2 * ts * 64;
        px += ts * 4;
    };
    auto park_h = [&](int u2, int i) {                   // f16 -> f32 weight scales of tiles i, i + 1 into their LDS slots
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const uint32_t hh = Hr[m][u2];
            *reinterpret_cast<float2*>(&wsl[(((i + (lane >> 5)) & 3) * NM + m) * 64 + 2 * (lane & 31)]) =
                make_float2(h2f((uint16_t)(hh & 0xffff)), h2f((uint16_t)(hh >> 16)));
        }
    };
    auto park_x = [&](int u, int i) { *reinterpret_cast<float2*>(&xsl[(i & 3) * 128 + (g >> 1) * 64 + 4 * t + 2 * (g & 1)]) = make_float2(Xr[u], Xr[u]); };
    // 16 B per lane (two blocks x one half) -> lo = 8 B of block 2j, hi = 8 B of block 2j + 1 for all four k-groups:
    // v_permlane32_swap exchanges lo[lanes 32-63] with hi[lanes 0-31]
    auto split = [](const v4i_t v, long& lo, long& hi) {
        const auto r0 = __builtin_amdgcn_permlane32_swap((unsigned)v[0], (unsigned)v[2], false, false);
        const auto r1 = __builtin_amdgcn_permlane32_swap((unsigned)v[1], (unsigned)v[3], false, false);
        lo = (long)(((unsigned long)r1[0] << 32) | r0[0]);
        hi = (long)(((unsigned long)r1[1] << 32) | r0[1]);
    };
    v2f_t acc[NM][2];
#pragma unroll
    for (int m = 0; m < NM; ++m) { acc[m][0] = v2f_t{0.f, 0.f}; acc[m][1] = v2f_t{0.f, 0.f}; }
    const v4i_t cbias = {0x4B400000, 0x4B400000, 0x4B400000, 0x4B400000};      // 1.5 * 2^23: int accumulator read as float = bias + isum
    const v2f_t fbias = {12582912.f, 12582912.f};
    v4i_t Cb[2][NM][4]; float4 Wc[NM][4]; v2f_t Xc[4];
    auto scales = [&](int i) {                           // weight / activation scales of tile i: LDS -> Wc / Xc
        const float4 x01 = *reinterpret_cast<const float4*>(&xsl[(i & 3) * 128 + 4 * t]), x23 = *reinterpret_cast<const float4*>(&xsl[(i & 3) * 128 + 64 + 4 * t]);
        Xc[0] = v2f_t{x01.x, x01.y}; Xc[1] = v2f_t{x01.z, x01.w}; Xc[2] = v2f_t{x23.x, x23.y}; Xc[3] = v2f_t{x23.z, x23.w};
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int bi = 0; bi < 4; ++bi) Wc[m][bi] = *reinterpret_cast<const float4*>(&wsl[((i & 3) * NM + m) * 64 + 16 * bi + 4 * g]);
    };
    auto front = [&](int u) {                            // ring slot u: swaps + 4 MFMAs per matrix -> Cb[u & 1]
        const int q = u & 1;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const long blo = Br[u][jj][0], bhi = Br[u][jj][1];
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                long alo, ahi;
                split(Ar[m][u][jj], alo, ahi);
                Cb[q][m][2 * jj] = __builtin_amdgcn_mfma_i32_16x16x32_i8(alo, blo, cbias, 0, 0, 0);         // block 2jj: the low registers
                Cb[q][m][2 * jj + 1] = __builtin_amdgcn_mfma_i32_16x16x32_i8(ahi, bhi, cbias, 0, 0, 0);     // block 2jj + 1: the high registers
            }
        }
    };
    // FULL is compile-time (no per-block branches in the full trips); nvalid < 4 only for the partial last tile of a K that is
    // not a multiple of 128
    auto back = [&](auto full_tag, int u, int nvalid) {
        constexpr bool FULL = decltype(full_tag)::value;
        const int q = u & 1;
#pragma unroll
        for (int bi = 0; bi < 4; ++bi) {
            if (!FULL && bi >= nvalid) continue;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const v4i_t c = Cb[q][m][bi];
                const float4 w4 = Wc[m][bi];
                const v2f_t ca = v2f_t{__int_as_float(c[0]), __int_as_float(c[1])} - fbias;
                const v2f_t cb = v2f_t{__int_as_float(c[2]), __int_as_float(c[3])} - fbias;
                acc[m][0] = acc[m][0] + ca * (v2f_t{w4.x, w4.y} * Xc[bi]);      // result += isum * (wScale * aScale)
                acc[m][1] = acc[m][1] + cb * (v2f_t{w4.z, w4.w} * Xc[bi]);
            }
        }
    };
    // prologue: the steady state's issue order
#pragma unroll
    for (int u = 0; u < DA; ++u) { fetch(u); __builtin_amdgcn_sched_barrier(0); }
    park_h(0, 0);
    park_x(0, 0);
    front(0);
    const int nfull = a.nb >> 2;                         // full tiles
    int base = 0;
    for (; base + DA <= nfull; base += DA) {             // full trips: branch-free
#pragma unroll
        for (int u = 0; u < DA; ++u) {
            const int i = base + u;
            scales(i);
            if ((u & 1) == 0) park_h(((u + 2) % DA) / 2, i + 2);               // scales of tiles i + 2, i + 3 (fetched DA - 2 tiles ago)
            park_x((u + 1) % DA, i + 1);
            front((u + 1) % DA);
            back(std::true_type{}, u, 4);
            fetch(u);
            __builtin_amdgcn_sched_barrier(0);           // or the scheduler hoists a later tile's swaps to just behind their loads (vmcnt(0))
        }
    }
    if (base < ntiles) {
        // last, partial trip: same straight-line schedule (fetches unconditional, no loop exits); only the arithmetic of tiles /
        // blocks past the end is skipped
#pragma unroll
        for (int u = 0; u < DA; ++u) {
            const int i = base + u;
            if (i < ntiles) {
                scales(i);
                if ((u & 1) == 0) park_h(((u + 2) % DA) / 2, i + 2);
                park_x((u + 1) % DA, i + 1);
                front((u + 1) % DA);
                back(std::false_type{}, u, min(4, a.nb - 4 * i));
                fetch(u);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#ifdef BDW_TIMING
    // per-wavefront record: where it ran (XCC, SE, CU, SIMD of HW_ID), when it started (100 MHz wall clock) and how many cycles its K walk took
    if (lane == 0) {
        const unsigned hw = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11)), xcc = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (3 << 11));
        printf("bdw EPI %d rows %d nb %d wg %d xcc %u se %u cu %u simd %u start %llu cycles %llu\n", EPI, a.rows, a.nb, (int)blockIdx.x, xcc & 15, (hw >> 13) & 7, (hw >> 8) & 15,
               (hw >> 4) & 3, bdw_w0, __builtin_readcyclecounter() - bdw_t0);
    }
#endif
    // epilogue.  C layout: token = 16 h + (lane & 15), weight rows 4g .. 4g + 3 of the strip
    const int b = 16 * h + t;
    if constexpr (QOUT) {
        // hb = silu(gate) * up leaves the kernel as the down projection's int8 operand (Q8_0FloatTensor.java:96-118): the two
        // wavefronts hold the 32 rows of one activation block for 16 tokens; block maximum through LDS, then every lane packs
        // its four rows = one quad of the block.  The f32 hb is not written (nothing else reads it on this path).
        float hv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float gt = acc[0][i >> 1][i & 1];
            gt = gt / (float)(1.0 + exp(-(double)gt));
            hv[i] = gt * acc[NM - 1][i >> 1][i & 1];
        }
        amax_s[wv][lane] = fmaxf(fmaxf(fabsf(hv[0]), fabsf(hv[1])), fmaxf(fabsf(hv[2]), fabsf(hv[3])));
        __syncthreads();
        float amax = 0.f;
#pragma unroll
        for (int w = 0; w < 2; ++w)
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) amax = fmaxf(amax, amax_s[w][16 * gg + t]);
        if (b >= a.ntok) return;
        const float qs = amax / 127.0f;
        const float ainv = qs != 0.f ? 1.0f / qs : 0.f;
        uint32_t packed = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float sv = hv[i] * ainv;
            packed |= (uint32_t)((int)(sv + copysignf(0.5f, sv)) & 0xFF) << (8 * i);
        }
        const int blk = strip >> 1;
        *reinterpret_cast<uint32_t*>(a.XQo + bdq_offset(blk * 8 + (strip & 1) * 4 + g, b, TS)) = packed;
        if (wv == 0 && g == 0) a.XSo[bds_offset(blk, b, TS)] = (float)(_Float16)qs;
        return;
    }
    if (GRP ? t >= gcnt : b >= a.ntok) return;
    const int rbase = (GRP ? unit : strip) * 16 + 4 * g;                        // GRP: row of the expert's own output
    const int orow = GRP ? (a.gdst ? a.gdst[gslot] : gslot) : b;
    float* o = a.out + (size_t)orow * a.out_stride + rbase;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (rbase + i >= a.rows) continue;
        const float v0 = acc[0][i >> 1][i & 1];
        if (EPI == EPI_SWIGLU) {
            float gt = v0;
            gt = gt / (float)(1.0 + exp(-(double)gt));
            o[i] = gt * acc[NM - 1][i >> 1][i & 1];
        } else if (EPI == EPI_STORE) o[i] = v0 * a.out_scale;
        else o[i] = o[i] + v0 * a.out_scale;
    }
}
