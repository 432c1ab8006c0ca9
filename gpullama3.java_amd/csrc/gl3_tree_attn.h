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
// pf_attn_softmax_pv_tree_kernel: the masked form of pf_attn_softmax_pv_kernel behind pf_attn_scores_kernel (run over [0, slot]) for every
// other shape and depth, the windowed branch for rows longer than the LDS window included.
#pragma once

constexpr int TA_TB = 8;
static_assert(TA_TB == FA_TB, "tree tiles are cut like the run table's");
__host__ __device__ constexpr size_t ta_smem_bytes(int hs, int group, int sstride) {
    return ((size_t)group * TA_TB * sstride + 2 * 64 * (hs + 4) + 64 + (size_t)group * TA_TB * hs) * 4;
}

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
