// gl3_tree_attn.h — attention of a draft-TREE verification step (gl3_forward_batch_verify_tree; compiled in gl3_prefill.hip, dispatch:
// pf_attention_tree()).
//
// A tree of `rows` step rows hangs off a sequence whose last real token sits at position p0.  Row i of the tree (first row row0) keeps its
// K / V row in the cache at SLOT p0 + (i - row0) — siblings share a position, never a slot — roped with its true position
// (pf_rope_kv_kernel: RopeArgs::slot).  A row sees the prefix [0, p0) and, of the tree's slots, those of its ancestors and itself: bit s of
// its 64-bit mask says "slot p0 + s is visible".  A parent precedes its children, so a row's visible slots ascend along its root path and
// end at its own slot: over the VISIBLE timesteps in ascending order every row computes what pf_attn_scores_kernel /
// pf_attn_softmax_pv_kernel compute for the linear run along its root path, element for element:
//   score     the sequential f32 mul-add over head_size, then / sqrt(head_size) (or * att_mul)
//   maximum   over the visible scores only
//   e         (float)exp((double)(s - max)); a masked timestep enters the strictly sequential sum as +0f (x + 0f == x exactly, and the
//             numerators are non-negative, so no -0f can appear)
//   weighted V sum   acc = w * v + acc over the visible timesteps ascending; a masked timestep is SKIPPED by predicate, never multiplied
//             by zero: the V row in a sibling's slot is unrelated data (it may hold anything, an infinity included)
//
// pf_attn_tree_kernel<HS, G>: one launch for scores + softmax + weighted V sum of trees whose score rows fit LDS.
//   workgroup = (kv head, tree tile of up to TA_TB = 8 rows that never crosses a tree), 4 wavefronts; G = kvMul <= 4 query heads.
//   The tile record is the run-table record of the one-launch prefill kernels {first row, rows, sequence, SLOT of the first row}: "row b
//   sits at slot pos0 + b" is then fa_tile's prologue unchanged.
//   LDS   Ssc [G][8][sstride]   score -> weight rows of the tile's (head, row) pairs
//         kt  [2][64][HS + 4]   K (phase 1) / V (phase 3) tiles of 64 timesteps, double-buffered: staged ONCE per tile for all 8 rows and all
//                               G heads (FA_FETCH / FA_PARK: the next tile's global loads are in flight under the current tile's arithmetic)
//         qs  [G][8][HS]        the tile's query rows
//   phase 1  wavefront w = rows 2w, 2w + 1 of the tile; lane = timestep of the K tile; the two rows' chains of every head run side by
//            side, 16 elements per trip: the lane's K row from LDS against broadcast reads of the query rows.  Scores of masked timesteps are computed and ignored.
//   phase 2  a wavefront per (head, row): masked maximum, e; then lane = row of wavefront 0: the sequential sums side by side
//            (seq_sum_lds_ring); divide.
//   phase 3  wavefront w = rows 2w, 2w + 1, lane = column(s); the prefix timesteps in groups of four without a mask, the tree's slots one
//            by one under the rows' mask bits (wavefront-uniform branches).
// The tiled form past that depth (and for the shapes without a one-launch kernel: kvMul 5 - 16, head size 96): the long-context trio with the
// score rows in HBM, three launches that share the prefix [0, p0) among a tree's rows instead of re-reading K and V once per row.
//   scores   the table forms of pf_scores_mfma_kernel / pf_scores_pk_kernel / pf_scores_tiled_kernel UNCHANGED over the tree tiles (the record
//            above is theirs): row b gets its scores over [0, slot], those of masked slots included.  The TMX entries of the 64-timestep tiles
//            that reach into [p0, slot] therefore fold masked scores: nothing reads them.
//   pf_softmax_rows_tree_kernel<R>   the masked pf_softmax_rows_kernel: maximum = TMX over the tiles wholly below p0 + ATT under the mask behind
//            them; e written back in place (masked: 0f) and streamed through LDS to the chain wavefront (lane = row, seq_sum_lds_ring); the
//            denominators go to SUMS, the division happens where the weights are staged.
//   pf_pv_tree_kernel<HS>   workgroup = (query head, up to PVT_TB = 16 rows of ONE tree — one p0), wavefront = 4 rows, lane = column(s).  V tiles of 64
//            timesteps and the rows' weights e / sum go through LDS once for all rows, the next tile in registers under the current tile's
//            arithmetic (pf_pv_ring_kernel's staging).  Prefix timesteps: PVR_TILE, no conditions; the tile that holds p0 is split there; the
//            tree's slots one by one under the rows' mask bits (wavefront-uniform branches).
// pf_attn_softmax_pv_tree_kernel: the masked form of pf_attn_softmax_pv_kernel behind pf_attn_scores_kernel (run over [0, slot]) for every
// step the other two forms do not take (pf_attention_tree), the windowed branch for rows longer than the LDS window included.
#pragma once

constexpr int TA_TB = 8;
static_assert(TA_TB == FA_TB, "tree tiles are cut like the run table's");
__host__ __device__ constexpr size_t ta_smem_bytes(int hs, int group, int sstride) {
    return ((size_t)group * TA_TB * sstride + 2 * 64 * (hs + 4) + 64 + (size_t)group * TA_TB * hs) * 4;
}
// pf_pv_tree_kernel: 4 wavefronts of 4 rows, so a tree of 64 rows is 4 workgroups per head.  (8 wavefronts — a V tile staged once for 32 rows —
// put two wavefronts on every SIMD of 64 workgroups where the launch is bound by the VALU: 248 us against 174 us per layer at depth 4096,
// profiles/spec_tree.md.)  LDS: a V tile [64][hs], then the weights [PVT_TB rows][64] of the tile.
constexpr int PVT_NW = 4, PVT_TB = 4 * PVT_NW, PVT_PER_TREE = 64 / PVT_TB;
__host__ __device__ constexpr size_t pv_tree_smem_bytes(int hs) { return (size_t)64 * (hs + PVT_TB) * 4; }

__device__ __forceinline__ bool tree_visible(int ts, int p0, unsigned long long mask) { return ts < p0 || ((mask >> (ts - p0)) & 1ull); }

template <int HS, int G>
__global__ __launch_bounds__(256) void pf_attn_tree_kernel(const float* __restrict__ Q, int q_stride, const float* __restrict__ kc, const float* __restrict__ vc,
                                                           float* __restrict__ out, int out_stride, int n_kv_heads, int kv_dim, float att_mul, int sstride,
                                                           const int4* __restrict__ tab, const int32_t* __restrict__ p0v,
                                                           const unsigned long long* __restrict__ maskv, size_t seq_stride) {
    extern __shared__ __attribute__((aligned(16))) float fa_sm[];
    constexpr int PITCH = HS + 4, H4 = HS / 4, NCOL = HS > 64 ? 2 : 1;
    float* Ssc = fa_sm;                                             // [G][TA_TB][sstride]
    float* kt = fa_sm + (size_t)G * TA_TB * sstride;                // [2][64][PITCH]
    float* sums = kt + 2 * 64 * PITCH;                              // [G * TA_TB] (+ padding to 64 floats)
    float* qs = sums + 64;                                          // [G][TA_TB][HS]
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const FaTile ft = fa_tile<true>(n_kv_heads, 0, 0, tab, seq_stride);
    const int kvh = ft.kvh, b0 = ft.b0, nb = ft.nb, pos0 = ft.pos0;      // row b of the tile sits at slot pos0 + b
    kc += ft.cache_off; vc += ft.cache_off;
    const int tmax = pos0 + b0 + nb - 1;                            // the tile's last slot: nothing behind it is visible to any of its rows
    const int p0 = __builtin_amdgcn_readfirstlane(p0v[b0]);         // one tree per tile
    const float sqrt_hs = (float)sqrt((double)HS);
    // this wavefront's two rows in phases 1 and 3 (the second clamped: computed again, stored nowhere)
    const int ra = 2 * wave, rb = min(2 * wave + 1, nb - 1);
    const bool wlive = ra < nb, rb_real = 2 * wave + 1 < nb;

    // ---- phase 1: scores
    float4 pk0, pk1, pk2, pk3, pk4, pk5, pk6, pk7;           // the staging registers of FA_FETCH / FA_PARK
    FA_FETCH(kc, t, 256, 0, min(64, tmax + 1));
    for (int i = t; i < G * TA_TB * H4; i += 256) {
        const int c = i % H4, tb = (i / H4) % TA_TB, hq = i / (H4 * TA_TB);
        *reinterpret_cast<float4*>(qs + (size_t)(hq * TA_TB + tb) * HS + 4 * c) =
            *reinterpret_cast<const float4*>(Q + (size_t)(b0 + min(tb, nb - 1)) * q_stride + (size_t)(kvh * G + hq) * HS + 4 * c);
    }
    int vb = 0;
    for (int t0 = 0; t0 <= tmax; t0 += 64, vb ^= 1) {
        const int tt = min(64, tmax + 1 - t0);
        float* ktile = kt + vb * 64 * PITCH;
        FA_PARK(ktile, t, 256);
        __syncthreads();                                             // (the first one also orders the query rows)
        FA_FETCH(kc, t, 256, min(t0 + 64, tmax), max(1, min(64, tmax + 1 - (t0 + 64))));
        if (!wlive) continue;
        const float4* krow = reinterpret_cast<const float4*>(ktile + min(lane, tt - 1) * PITCH);      // the lane's K row
        const int ts = t0 + lane;
#pragma unroll 1
        for (int hq = 0; hq < G; ++hq) {
            const float4* qa = reinterpret_cast<const float4*>(qs + (size_t)(hq * TA_TB + ra) * HS);
            const float4* qb = reinterpret_cast<const float4*>(qs + (size_t)(hq * TA_TB + rb) * HS);
            float s0 = 0.f, s1 = 0.f;
            // 16 elements per trip: the K row comes from LDS again for every head (64 distinct addresses, the full LDS rate) instead of
            // living in HS registers beside 2 HS products in flight
#pragma unroll 1
            for (int c0 = 0; c0 < H4; c0 += 4) {
#pragma unroll
                for (int c = c0; c < c0 + 4; ++c) {
                    const float4 a = qa[c], b = qb[c], k = krow[c];
                    s0 = s0 + a.x * k.x; s1 = s1 + b.x * k.x;
                    s0 = s0 + a.y * k.y; s1 = s1 + b.y * k.y;
                    s0 = s0 + a.z * k.z; s1 = s1 + b.z * k.z;
                    s0 = s0 + a.w * k.w; s1 = s1 + b.w * k.w;
                }
            }
            if (lane < tt) {
                if (ts <= pos0 + b0 + ra) Ssc[(size_t)(hq * TA_TB + ra) * sstride + ts] = att_mul != 0.f ? s0 * att_mul : s0 / sqrt_hs;
                if (rb_real && ts <= pos0 + b0 + rb) Ssc[(size_t)(hq * TA_TB + rb) * sstride + ts] = att_mul != 0.f ? s1 * att_mul : s1 / sqrt_hs;
            }
        }
    }
    __syncthreads();                                                 // every score row is written; both tile buffers are free

    // the first V tile travels while the softmax runs
    FA_FETCH(vc, t, 256, 0, min(64, tmax + 1));
    // ---- phase 2: softmax of the G * nb rows over their visible timesteps
    const int nrows = G * nb;
    for (int row = wave; row < nrows; row += 4) {
        const int tb = row % nb, n = pos0 + b0 + tb + 1;
        const unsigned long long mask = maskv[b0 + tb];
        float* e = Ssc + (size_t)((row / nb) * TA_TB + tb) * sstride;
        float mx = -INFINITY;
        for (int i = lane; i < n; i += 64) if (tree_visible(i, p0, mask)) mx = fmaxf(mx, e[i]);
        mx = wave_max(mx);
        for (int i = lane; i < n; i += 64) e[i] = tree_visible(i, p0, mask) ? (float)exp((double)(e[i] - mx)) : 0.f;
    }
    __syncthreads();
    if (wave == 0 && lane < nrows) {
        const int tb = lane % nb, n = pos0 + b0 + tb + 1;
        sums[lane] = seq_sum_lds_ring(Ssc + (size_t)((lane / nb) * TA_TB + tb) * sstride, n);
    }
    __syncthreads();
    for (int row = wave; row < nrows; row += 4) {
        const int tb = row % nb, n = pos0 + b0 + tb + 1;
        float* e = Ssc + (size_t)((row / nb) * TA_TB + tb) * sstride;
        const float sum = sums[row];
        for (int i = lane; i < n; i += 64) e[i] = e[i] / sum;
    }

    // ---- phase 3: weighted V sum
    const unsigned long long mka = maskv[b0 + min(ra, nb - 1)], mkb = maskv[b0 + rb];
    const float* wa = Ssc + (size_t)min(ra, nb - 1) * sstride;       // + hq * TA_TB * sstride: the head's rows
    const float* wb = Ssc + (size_t)rb * sstride;
    float acc[G][2][NCOL];
#pragma unroll
    for (int hq = 0; hq < G; ++hq)
#pragma unroll
        for (int c = 0; c < NCOL; ++c) acc[hq][0][c] = acc[hq][1][c] = 0.f;
    vb = 0;
    for (int t0 = 0; t0 <= tmax; t0 += 64, vb ^= 1) {
        const int tt = min(64, tmax + 1 - t0);
        const float* vt = kt + vb * 64 * PITCH;
        FA_PARK(kt + vb * 64 * PITCH, t, 256);
        __syncthreads();                                             // (also orders phase 2's writes before the first reads of the weights)
        FA_FETCH(vc, t, 256, min(t0 + 64, tmax), max(1, min(64, tmax + 1 - (t0 + 64))));
        if (!wlive) continue;
        const float* vp = vt + (NCOL == 2 ? 2 * lane : min(lane, HS - 1));
        // acc = w * v + acc for this lane's column(s) of V row R_ (a macro: a register array captured by a lambda ends up in scratch)
#define TA_STEP(R_, HQ_, U_, W_) do { const float w_ = (W_); \
            if (NCOL == 2) { const float2 v2_ = *reinterpret_cast<const float2*>(vp + (R_) * PITCH); \
                acc[HQ_][U_][0] = w_ * v2_.x + acc[HQ_][U_][0]; acc[HQ_][U_][NCOL - 1] = w_ * v2_.y + acc[HQ_][U_][NCOL - 1]; } \
            else acc[HQ_][U_][0] = w_ * vp[(R_) * PITCH] + acc[HQ_][U_][0]; } while (0)
        const int npre = max(0, min(tt, p0 - t0));                   // timesteps of this tile in the prefix: visible to every row
        int r = 0;
        for (; r + 4 <= npre; r += 4)
#pragma unroll
            for (int hq = 0; hq < G; ++hq) {
                const float4 a4 = *reinterpret_cast<const float4*>(wa + (size_t)hq * TA_TB * sstride + t0 + r);
                const float4 b4 = *reinterpret_cast<const float4*>(wb + (size_t)hq * TA_TB * sstride + t0 + r);
                TA_STEP(r, hq, 0, a4.x); TA_STEP(r, hq, 1, b4.x);
                TA_STEP(r + 1, hq, 0, a4.y); TA_STEP(r + 1, hq, 1, b4.y);
                TA_STEP(r + 2, hq, 0, a4.z); TA_STEP(r + 2, hq, 1, b4.z);
                TA_STEP(r + 3, hq, 0, a4.w); TA_STEP(r + 3, hq, 1, b4.w);
            }
        for (; r < tt; ++r) {                                        // the prefix' last timesteps, then the tree's slots under the mask
            const bool va = tree_visible(t0 + r, p0, mka), vb2 = tree_visible(t0 + r, p0, mkb);
#pragma unroll
            for (int hq = 0; hq < G; ++hq) {
                if (va) TA_STEP(r, hq, 0, wa[(size_t)hq * TA_TB * sstride + t0 + r]);
                if (vb2) TA_STEP(r, hq, 1, wb[(size_t)hq * TA_TB * sstride + t0 + r]);
            }
        }
    }
#undef TA_STEP
    if (!wlive) return;
#pragma unroll
    for (int hq = 0; hq < G; ++hq)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u == 1 && !rb_real) continue;
            float* o = out + (size_t)(b0 + (u ? rb : ra)) * out_stride + (size_t)(kvh * G + hq) * HS;
            if (NCOL == 2) *reinterpret_cast<float2*>(o + 2 * lane) = make_float2(acc[hq][u][0], acc[hq][u][NCOL - 1]);
            else if (lane < HS) o[lane] = acc[hq][u][0];
        }
}

// The masked pf_attn_softmax_pv_kernel: grid = (n_heads * ceil(hs / 64), ntok), block = 64; a.pos = the rows' SLOTS (the scores kernel ran over
// [0, slot]), a.win = floats of a row held in LDS.  Same phases, same windows; a masked timestep is +0f in the sum and skipped in the V sum.
__global__ __launch_bounds__(64) void pf_attn_softmax_pv_tree_kernel(const PfAttnArgs a, const int32_t* __restrict__ p0v, const unsigned long long* __restrict__ maskv) {
    extern __shared__ __attribute__((aligned(16))) float e_s[];
    const int hs = a.hs, kvmul = a.n_heads / a.n_kv_heads;
    const int nj = (hs + 63) / 64;
    const int h = blockIdx.x / nj, j = (blockIdx.x % nj) * 64 + threadIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x, kvh = h / kvmul;
    const int n = a.pos[b] + 1, W = a.win, p0 = p0v[b];
    const unsigned long long mask = maskv[b];
    const float* sc = a.att + ((size_t)b * a.n_heads + h) * a.ctx;
    float mx = -INFINITY;
    for (int i = lane; i < n; i += 64) if (tree_visible(i, p0, mask)) mx = fmaxf(mx, sc[i]);
    mx = wave_max(mx);
    float sum = 0.f;
    if (n <= W) {
        for (int i = lane; i < n; i += 64) e_s[i] = tree_visible(i, p0, mask) ? (float)exp((double)(sc[i] - mx)) : 0.f;
        __syncthreads();
        sum = seq_sum_lds<false>(e_s, n);
        __syncthreads();
        for (int i = lane; i < n; i += 64) e_s[i] = e_s[i] / sum;
        __syncthreads();
    } else {
        for (int c0 = 0; c0 < n; c0 += W) {
            const int len = min(W, n - c0);
            __syncthreads();
            for (int i = lane; i < len; i += 64) e_s[i] = tree_visible(c0 + i, p0, mask) ? (float)exp((double)(sc[c0 + i] - mx)) : 0.f;
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
            for (int i = lane; i < clen; i += 64) e_s[i] = tree_visible(c0 + i, p0, mask) ? (float)exp((double)(sc[c0 + i] - mx)) / sum : 0.f;
            __syncthreads();
        }
        const float* vw = v + (size_t)c0 * a.kv_dim;
        const int npre = max(0, min(clen, p0 - c0));     // prefix timesteps of this window: no mask
        int tt = 0;
        for (; tt + 8 <= npre; tt += 8) {
            float vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) vv[u] = vw[(size_t)(tt + u) * a.kv_dim];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = e_s[tt + u] * vv[u] + acc;
        }
        for (; tt < clen; ++tt)
            if (tree_visible(c0 + tt, p0, mask)) acc = e_s[tt] * vw[(size_t)tt * a.kv_dim] + acc;
    }
    if (j < hs) a.out[(size_t)b * a.out_stride + h * hs + j] = acc;
}

// The masked pf_softmax_rows_kernel (the tiled form's second launch): R score rows per workgroup, 8 worker wavefronts that stream the rows'
// 64-timestep tiles a tile ahead, a ninth wavefront with lane = row on the strictly sequential sums.  Score row i = (step row i / n_heads, head
// i % n_heads) of ALL rows of the step; a.pos = the rows' SLOTS (a row is slot + 1 long).
//   maximum   8 lanes per row: TMX over the tiles wholly below the row's p0 (every timestep there is visible), then the scores from the first
//             tile that reaches p0 to the row's slot out of ATT under the mask (at most 64 + 63 of them)
//   e         (float)exp((double)(s - max)) where visible, 0f where masked or behind the row's end: in place and into the LDS tile
//   sum       over [0, slot] ascending, a masked timestep as +0f -> SUMS
template <int R>
__global__ __launch_bounds__(576) void pf_softmax_rows_tree_kernel(const PfAttnArgs a, int nrows_total, const float* __restrict__ tmx, int tmx_tiles, float* __restrict__ sums,
                                                                   const int32_t* __restrict__ p0v, const unsigned long long* __restrict__ maskv) {
    __shared__ __attribute__((aligned(16))) float E[2][R * SR_PITCH];
    __shared__ float mx_s[R];
    __shared__ int n_s[R];
    __shared__ int p0_s[R];
    __shared__ unsigned long long mask_s[R];
    __shared__ int nmax_s;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int row0 = blockIdx.x * R;
    if (t == 0) nmax_s = 0;
    if (t < R * 8) {
        const int r = t >> 3, sub = t & 7, row = min(row0 + r, nrows_total - 1), b = row / a.n_heads;
        const int n = row0 + r < nrows_total ? a.pos[b] + 1 : 0, p0 = p0v[b];
        const unsigned long long mask = maskv[b];
        const int nfull = min(p0, n) >> 6;            // tiles wholly inside the prefix
        const float* sc = a.att + (size_t)row * a.ctx;
        float m = -INFINITY;
        for (int i = sub; i < nfull; i += 8) m = fmaxf(m, tmx[(size_t)row * tmx_tiles + i]);
        for (int i = 64 * nfull + sub; i < n; i += 8) if (tree_visible(i, p0, mask)) m = fmaxf(m, sc[i]);
        m = row8_max(m);
        if (sub == 0) { mx_s[r] = m; n_s[r] = n; p0_s[r] = p0; mask_s[r] = mask; }
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
        if (lane < R && row0 + lane < nrows_total) sums[row0 + lane] = s;
        return;
    }
    constexpr int NS = (R * 16 + 511) / 512;          // 16-byte slots per worker thread and tile
    float* rowp[NS]; float mrow[NS]; int nrow[NS], ldsoff[NS], prow[NS]; unsigned long long krow[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const int q = min(t + 512 * u, R * 16 - 1), r = q >> 4, c4 = q & 15;
        rowp[u] = a.att + (size_t)min(row0 + r, nrows_total - 1) * a.ctx + 4 * c4;
        mrow[u] = mx_s[r];
        nrow[u] = (t + 512 * u < R * 16) ? n_s[r] - 4 * c4 : 0;       // elements of the row at and behind this slot's first column of tile 0
        prow[u] = p0_s[r] - 4 * c4;                                   // prefix timesteps likewise
        krow[u] = mask_s[r];
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
            const int left = nrow[u] - 64 * k;        // elements of the row from this slot's first on: element j exists when left > j
            const int d = 64 * k - prow[u];           // element j is tree slot d + j of the row's tree (< 0: prefix); left > j implies d + j < 64
            const float x[4] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                e[j] = left > j && (d + j < 0 || ((krow[u] >> (d + j)) & 1ull)) ? (float)exp((double)(x[j] - mrow[u])) : 0.f;
            const float4 e4 = make_float4(e[0], e[1], e[2], e[3]);
            if (t + 512 * u < R * 16) *reinterpret_cast<float4*>(&E[k & 1][ldsoff[u]]) = e4;
            if (left > 0) *reinterpret_cast<float4*>(rowp[u] + 64 * k) = e4;      // in place (columns past the row's end stay inside the row: ctx % 4 == 0)
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NS; ++u) cur[u] = nxt[u];
    }
}

// The weighted V sum of the tiled form on the VALU: grid = (n_heads, PVT_PER_TREE per tree), block = PVT_NW wavefronts of 4 rows; workgroup (h, y) serves rows
// [PVT_TB q, PVT_TB q + PVT_TB), q = y % PVT_PER_TREE, of tree y / PVT_PER_TREE (`trees`: {first row, rows, sequence, p0}) for query head h, lane = the output column(s):
// acc = w * v + acc over the row's visible timesteps ascending.  Staging as in pf_pv_ring_kernel: the next tile's V rows and numerators are
// requested into registers before the current tile is consumed and reach LDS (the numerators divided by the row's sum) behind it.  Per tile:
// the timesteps below p0 in groups of four through PVR_TILE (every row sees them: no conditions), the prefix' last one to three and the tree's
// slots one by one — a row takes a slot only where its mask bit is set, a branch on SGPRs: the V row in a sibling's slot is never multiplied, by
// zero or anything else.  (A row slot past the workgroup's last row carries zero weights through the prefix and stores nothing.)
template <int HS>
__global__ __launch_bounds__(64 * PVT_NW) void pf_pv_tree_kernel(const PfAttnArgs a, const float* __restrict__ sums, const int4* __restrict__ trees,
                                                                const unsigned long long* __restrict__ maskv) {
    constexpr int NCOL = HS > 64 ? 2 : 1, H4 = HS / 4, NT = 64 * PVT_NW, VPT = 64 * H4 / NT;
    static_assert(VPT * NT == 64 * H4, "a V tile is a whole number of 16-byte slots per thread");
    extern __shared__ __attribute__((aligned(16))) float vt[];        // [64][HS] V rows, then [PVT_TB][64] weights
    float* as = vt + 64 * HS;
    const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int4 rec = trees[blockIdx.y / PVT_PER_TREE];
    const int half = blockIdx.y % PVT_PER_TREE, p0 = __builtin_amdgcn_readfirstlane(rec.w);
    const int b0 = __builtin_amdgcn_readfirstlane(rec.x) + PVT_TB * half, nb = min(PVT_TB, __builtin_amdgcn_readfirstlane(rec.y) - PVT_TB * half);
    if (nb <= 0) return;                                              // the tree ends before this piece
    const int slot0 = p0 + PVT_TB * half;                             // row tb of the workgroup sits at slot slot0 + tb
    const int tmax = slot0 + nb - 1, ntile = tmax / 64 + 1;
    const int kvmul = a.n_heads / a.n_kv_heads, h = blockIdx.x, kvh = h / kvmul;
    const bool wlive = 4 * w < nb;
    const int wlast = slot0 + min(4 * w + 3, nb - 1);                 // last slot any of this wavefront's four rows sees
    const float* vc = a.vcache + (size_t)__builtin_amdgcn_readfirstlane(rec.z) * a.seq_stride + kvh * HS;
    unsigned long long mk[4];                                         // the wavefront's rows' masks (SGPRs)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned long long m = 4 * w + u < nb ? maskv[b0 + 4 * w + u] : 0ull;
        mk[u] = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(m >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)m);
    }
    // staging roles: thread = (row w + PVT_NW j, timestep lane) of the weights; 16-byte slots t + NT j of the V tile
    const float* arow[4]; float rsum[4]; int apos[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tb = w + PVT_NW * j;
        apos[j] = tb < nb ? slot0 + tb : -1;
        arow[j] = a.att + ((size_t)(b0 + min(tb, nb - 1)) * a.n_heads + h) * a.ctx;
        rsum[j] = sums[(size_t)(b0 + min(tb, nb - 1)) * a.n_heads + h];
    }
    typedef float v4f_native __attribute__((ext_vector_type(4)));
    v4f_native vreg[VPT]; float areg[4];
#define PVT_GLOAD(K_) do { const int t0_ = 64 * (K_); \
        static_for<0, VPT, 1>([&](auto jc) { constexpr int j = decltype(jc)::value; const int i = t + NT * j, r = i / H4, c = i % H4; \
            vreg[j] = *reinterpret_cast<const v4f_native*>(vc + (size_t)min(t0_ + r, tmax) * a.kv_dim + 4 * c); }); \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) areg[j] = arow[j][max(min(t0_ + lane, apos[j]), 0)]; } while (0)
#define PVT_LSTORE(K_) do { const int t0_ = 64 * (K_); \
        static_for<0, VPT, 1>([&](auto jc) { constexpr int j = decltype(jc)::value; const int i = t + NT * j, r = i / H4, c = i % H4; \
            *reinterpret_cast<v4f_native*>(vt + r * HS + 4 * c) = vreg[j]; }); \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) as[(w + PVT_NW * j) * 64 + lane] = t0_ + lane <= apos[j] ? areg[j] / rsum[j] : 0.f; } while (0)
    float acc[4][NCOL];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < NCOL; ++c) acc[u][c] = 0.f;
    const float* vp = vt + (NCOL == 2 ? 2 * min(lane, HS / 2 - 1) : min(lane, HS - 1));      // lanes past the last column (head size 96, 32) repeat it and store nothing
    const float* ap = as + 4 * w * 64;
    PVT_GLOAD(0);
    PVT_LSTORE(0);
    __syncthreads();
    for (int k = 0; k < ntile; ++k) {
        PVT_GLOAD(min(k + 1, ntile - 1));                            // unconditional (a condition around the loads makes the compiler drain them)
        if (wlive) {
            const int t0 = 64 * k, npre = max(0, min(64, p0 - t0));  // prefix timesteps of the tile (p0 <= tmax: all of them are cache rows)
            PVR_TILE(npre >> 2, 64, HS);
            const int tend = min(64, wlast + 1 - t0);
            for (int r = npre & ~3; r < tend; ++r) {
                const int d = t0 + r - p0;                           // tree slot (0 .. 63), < 0: the prefix' last timesteps
                float vv[NCOL];
                if (NCOL == 2) { const float2 x = *reinterpret_cast<const float2*>(vp + r * HS); vv[0] = x.x; vv[NCOL - 1] = x.y; }
                else vv[0] = vp[r * HS];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (d < 0 || ((mk[u] >> d) & 1ull)) {
                        const float wt = ap[u * 64 + r];
#pragma unroll
                        for (int c = 0; c < NCOL; ++c) acc[u][c] = wt * vv[c] + acc[u][c];
                    }
            }
        }
        __syncthreads();
        PVT_LSTORE(min(k + 1, ntile - 1));
        __syncthreads();
    }
#undef PVT_GLOAD
#undef PVT_LSTORE
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
