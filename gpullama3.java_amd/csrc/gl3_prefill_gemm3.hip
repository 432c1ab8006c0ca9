// gl3_prefill_gemm3.hip — translation unit of pf_gemm3_kernel (gl3_prefill_gemm3.h) and pf_gemm3t_kernel (gl3_prefill_gemm3t.h), the
// batched-prefill Q8_0 GEMMs for > 64 tokens, and of the rules that pick a tiling per matrix shape.
// Separate from gl3_prefill.hip because it is compiled with -fno-slp-vectorize: the per-block arithmetic must stay scalar
// (v_fma_f32 / v_add_f32) — packed f32 instructions beside MFMAs are slow on gfx950, see gl3_prefill_gemm3.h.
#include "gl3_ctx.h"
#include <type_traits>
#include "gl3_decode_kernels.h"
using namespace gl3;
#include "gl3_bd_gemm.h"          // GemmArgs
#include "gl3_prefill_gemm3.h"
#include "gl3_prefill_gemm3t.h"

// Dynamic LDS above 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize (below it the call is harmless).  gl3_gemm3_allow_lds is called by
// gl3_prefill_alloc for every plan, after hipSetDevice, like the attributes of the other kernels: the attribute belongs to the
// (function, device) pair, and a once-per-process flag would leave a second device's plan — or a second in-process rank racing on
// the flag — without it.
template <int EPI, int RF, int TF, int WR, int WC, int KB>
constexpr int g3_lds_bytes() { return G3_RING * g3_stage_bytes((EPI == EPI_SWIGLU ? 2 : 1) * RF * 32 * WR, WC * TF * 32, KB); }
template <int EPI, int RF, int TF, int WR, int WC, int KB, int OCC>
static void g3_launch(const GemmArgs& a, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((pf_gemm3_kernel<EPI, RF, TF, WR, WC, KB, OCC>), grid, dim3(64 * WR * WC), (g3_lds_bytes<EPI, RF, TF, WR, WC, KB>()), s, a);
}
template <int EPI, int RF, int TF, int WR, int WC, int KB, int OCC>
static hipError_t g3_allow() {
    return hipFuncSetAttribute((const void*)pf_gemm3_kernel<EPI, RF, TF, WR, WC, KB, OCC>, hipFuncAttributeMaxDynamicSharedMemorySize, g3_lds_bytes<EPI, RF, TF, WR, WC, KB>());
}
// tile shapes (rows x tokens per workgroup; wavefront grid; blocks per stage):
//   BIG   128 x 128, 2 x 2 wavefronts of 2 x 2 fragments, KB 2, two workgroups per CU   (gate + up as 64 + 64 rows; matrices with >= 512 such tiles)
//   QKV    96 x 128, 3 x 4 one-tile wavefronts, KB 4, one workgroup per CU              (row counts that are a multiple of 96 with 128..384 tiles: 6144-row qkv)
//   SMALL  64 x 128, 2 x 4 one-tile wavefronts, KB 4, one workgroup per CU              (everything else: the 4096-row wo / down projections)
//   SMALL2 64 x 64,  2 x 2 one-tile wavefronts, KB 4, two workgroups per CU             (A/B: GL3_PF_GEMM3_SHAPE=4 — two independent barrier domains per CU)
template <int EPI>
static hipError_t g3_allow_epi() {
    hipError_t e = g3_allow<EPI, EPI == EPI_SWIGLU ? 1 : 2, 2, 2, 2, 2, 2>();
    if constexpr (EPI != EPI_SWIGLU) {
        if (e == hipSuccess) e = g3_allow<EPI, 1, 1, 3, 4, 4, 1>();
        if (e == hipSuccess) e = g3_allow<EPI, 1, 1, 2, 4, 4, 1>();
        if (e == hipSuccess) e = g3_allow<EPI, 1, 1, 2, 2, 4, 2>();
    }
    return e;
}
template <int NFR, int KBT>
static hipError_t g3t_allow() {
    hipError_t e = hipFuncSetAttribute((const void*)pf_gemm3t_kernel<NFR, KBT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, g3t_lds_bytes(NFR, KBT));
    if (e == hipSuccess && KBT == 2) e = hipFuncSetAttribute((const void*)pf_gemm3t_kernel<NFR, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, g3t_lds_bytes(NFR, 2));
    return e;
}
enum { G3K_GEMM3 = 0, G3K_GEMM3T = 1 };      // pf_gemm3_kernel, pf_gemm3t_kernel
struct G3Plan {
    int kernel, tile_rows, tile_tok, kb, nfr;      // workgroup tile: rows per matrix x tokens; blocks per K stage; tall row fragments (0: pf_gemm3_kernel)
    int nrt, ntt, grid, qout;                      // row tiles, token tiles, workgroups; 1 = the gate + up launch can write hb quantised
};
template <int NFR, int KBT>
static void g3t_launch(GemmArgs a, const G3Plan& pl, hipStream_t s) {
    a.ntt = pl.ntt; a.nrt = pl.nrt;
    const dim3 g(pl.grid);
    if (KBT == 2 && a.XPo) hipLaunchKernelGGL((pf_gemm3t_kernel<NFR, 2, true>), g, dim3(512), g3t_lds_bytes(NFR, 2), s, a);      // hb leaves the kernel quantised
    else hipLaunchKernelGGL((pf_gemm3t_kernel<NFR, KBT, false>), g, dim3(512), g3t_lds_bytes(NFR, KBT), s, a);
}
// The switches of the choice, read once per process.
struct G3Switches {
    int tall = 0;            // GL3_PF_GEMM3_TALL: -1 gate + up never on the tall tiling, 4 .. 7 that many row fragments always
    int tall_kb = 2;         // GL3_PF_GEMM3_TALL_KB: blocks per K stage of the tall tiling (1 | 2)
    int shape = 0;           // GL3_PF_GEMM3_SHAPE (A/B): 1 BIG, 2 QKV, 3 SMALL, 4 SMALL2 for every non-SwiGLU launch
    bool qout_off = false;   // GL3_PF_GEMM3_QOUT=0: hb stays f32 behind the tall tiling
};
static const G3Switches& g3_switches() {
    static const G3Switches sw = [] {
        G3Switches x;
        if (getenv("GL3_PF_GEMM3_TALL")) x.tall = atoi(getenv("GL3_PF_GEMM3_TALL"));
        if (getenv("GL3_PF_GEMM3_TALL_KB")) x.tall_kb = atoi(getenv("GL3_PF_GEMM3_TALL_KB"));
        if (getenv("GL3_PF_GEMM3_SHAPE")) x.shape = atoi(getenv("GL3_PF_GEMM3_SHAPE"));
        x.qout_off = getenv("GL3_PF_GEMM3_QOUT") && atoi(getenv("GL3_PF_GEMM3_QOUT")) == 0;
        return x;
    }();
    return sw;
}
// the tiling the gate + up launch of (rows, ntok) takes: 0 = 128 x 128, 4 .. 7 = tall with that many row fragments (gl3_prefill_gemm3t.h)
static int g3_tall_choice(int rows, int ntok, const G3Switches& sw) {
    const int ntt = (ntok + 127) / 128;
    int best = 0, cost = ((ntt * ((rows + 63) / 64) + 511) / 512) * 8;      // 128 x 128: two workgroups per CU, 8 result tiles per SIMD and round
    for (int nfr = 4; nfr <= 7 && sw.tall == 0; ++nfr) {                    // tall: one workgroup per CU, 2 NFR tiles per SIMD and round
        const int c = ((ntt * ((rows + 32 * nfr - 1) / (32 * nfr)) + 255) / 256) * 2 * nfr;
        if (c < cost) { cost = c; best = nfr; }
    }
    if (sw.tall >= 4 && sw.tall <= 7) best = sw.tall;
    return best;
}
// The one host-side choice of a > 64-token Q8_0 GEMM: which kernel, its workgroup tile, blocks per K stage, row and token tiles and the grid.
// g3_dispatch launches what the plan says, gl3_gemm3_swiglu_quantises reads its qout, and gl3_debug_gemm3_plan answers from the same
// function with no device, which is what tests/gemm3_shapes.py holds its Python restatement to.
//   gate + up (EPI_SWIGLU): the 128 x 128 tiling (64 + 64 rows) or a tall tiling of NFR = 4 .. 7 row fragments per matrix (gl3_prefill_gemm3t.h)
//   — whichever leaves a SIMD fewer tile-steps (g3_tall_choice; the first of equal costs stays, so NFR 4 needs the switch).
//   store / resid: 128 x 128 from 512 such tiles, 96 x 128 for row counts that 96 divides with more than 128 and at most 384 tiles, else 64 x 128.
// Every workgroup finds its tile by J = (lin & 7) * per_xcd + (lin >> 3) over a grid rounded up to 8; J >= nrt * ntt leaves at once.
static G3Plan g3_plan(int epi, int rows, int ntok, const G3Switches& sw) {
    G3Plan p{};
    p.kernel = G3K_GEMM3; p.tile_tok = 128; p.ntt = (ntok + 127) / 128;
    if (epi == EPI_SWIGLU) {
        p.nfr = g3_tall_choice(rows, ntok, sw);
        if (p.nfr) {
            p.kernel = G3K_GEMM3T; p.tile_rows = 32 * p.nfr; p.kb = sw.tall_kb == 1 ? 1 : 2;
            p.qout = !sw.qout_off && sw.tall_kb == 2 && rows % 32 == 0;      // the caller then passes XQo / XPo and skips the quantise launch
        } else { p.tile_rows = 64; p.kb = 2; }
    } else {
        const int t128 = p.ntt * ((rows + 127) / 128), t96 = p.ntt * ((rows + 95) / 96);
        const int shape = sw.shape ? sw.shape : t128 >= 512 ? 1 : (rows % 96 == 0 && t96 > 128 && t96 <= 384) ? 2 : 3;
        if (shape == 1) { p.tile_rows = 128; p.kb = 2; }
        else if (shape == 2) { p.tile_rows = 96; p.kb = 4; }
        else if (shape == 4) { p.tile_rows = 64; p.kb = 4; p.tile_tok = 64; p.ntt = (ntok + 63) / 64; }
        else { p.tile_rows = 64; p.kb = 4; }
    }
    p.nrt = (rows + p.tile_rows - 1) / p.tile_rows;
    p.grid = 8 * ((p.ntt * p.nrt + 7) / 8);
    return p;
}
// true when the gate + up launch can write hb quantised (pf_gemm3t_kernel<.., QOUT>): the caller then passes XQo / XPo and skips the quantise launch
bool gl3_gemm3_swiglu_quantises(int rows, int ntok) { return g3_plan(EPI_SWIGLU, rows, ntok, g3_switches()).qout != 0; }
int32_t gl3_debug_gemm3_plan(int32_t epi, int32_t rows, int32_t ntok, int32_t out[9]) {
    if (!out || rows < 1 || ntok < 1 || (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_SWIGLU)) return GL3_E_ARG;
    const G3Plan p = g3_plan(epi, rows, ntok, g3_switches());
    out[0] = p.kernel; out[1] = p.tile_rows; out[2] = p.tile_tok; out[3] = p.kb; out[4] = p.nfr; out[5] = p.nrt; out[6] = p.ntt; out[7] = p.grid; out[8] = p.qout;
    return GL3_OK;
}
hipError_t gl3_gemm3_allow_lds() {
    hipError_t e = g3_allow_epi<EPI_SWIGLU>();
    if (e == hipSuccess) e = g3t_allow<4, 1>();
    if (e == hipSuccess) e = g3t_allow<5, 1>();
    if (e == hipSuccess) e = g3t_allow<6, 1>();
    if (e == hipSuccess) e = g3t_allow<7, 1>();
    if (e == hipSuccess) e = g3t_allow<4, 2>();
    if (e == hipSuccess) e = g3t_allow<5, 2>();
    if (e == hipSuccess) e = g3t_allow<6, 2>();
    if (e == hipSuccess) e = g3t_allow<7, 2>();
    if (e == hipSuccess) e = g3_allow_epi<EPI_RESID>();
    if (e == hipSuccess) e = g3_allow_epi<EPI_STORE>();
    return e;
}
template <int EPI>
static void g3_dispatch(GemmArgs a, int rows, int ntok, hipStream_t s) {
    const G3Plan pl = g3_plan(EPI, rows, ntok, g3_switches());
    a.ntt = pl.ntt; a.nrt = pl.nrt;
    const dim3 grid(pl.grid);
    if constexpr (EPI == EPI_SWIGLU) {
        // gate + up: the 128 x 128 tiling or a tall tiling (gl3_prefill_gemm3t.h) — whichever leaves a SIMD fewer tile-steps (g3_tall_choice).
        // GL3_PF_GEMM3_TALL: -1 never, 4 .. 7 that shape always.
#define GL3_G3T(N_) do { if (pl.kb == 1) g3t_launch<N_, 1>(a, pl, s); else g3t_launch<N_, 2>(a, pl, s); } while (0)
        switch (pl.nfr) {
        case 4: GL3_G3T(4); break;
        case 5: GL3_G3T(5); break;
        case 6: GL3_G3T(6); break;
        case 7: GL3_G3T(7); break;
        default: g3_launch<EPI, 1, 2, 2, 2, 2, 2>(a, grid, s);
        }
#undef GL3_G3T
    } else {
        if (pl.tile_rows == 128) g3_launch<EPI, 2, 2, 2, 2, 2, 2>(a, grid, s);
        else if (pl.tile_rows == 96) g3_launch<EPI, 1, 1, 3, 4, 4, 1>(a, grid, s);
        else if (pl.tile_tok == 64) g3_launch<EPI, 1, 1, 2, 2, 4, 2>(a, grid, s);
        else g3_launch<EPI, 1, 1, 2, 4, 4, 1>(a, grid, s);
    }
}
void gl3_gemm3_launch(int epi, const GemmArgs& a, int rows, int ntok, hipStream_t s) {
    if (epi == EPI_SWIGLU) g3_dispatch<EPI_SWIGLU>(a, rows, ntok, s);
    else if (epi == EPI_RESID) g3_dispatch<EPI_RESID>(a, rows, ntok, s);
    else g3_dispatch<EPI_STORE>(a, rows, ntok, s);
}
