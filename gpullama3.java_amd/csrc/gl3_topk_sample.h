// gl3_topk_sample.h — top-k / min-p / top-p sampling over k survivors, one launch per step, one workgroup per row.
//
// The sampler other GGUF hosts default to: keep the k largest logits, cut by min-p and top-p, draw.  The reference has no such sampler, so
// its arithmetic is fixed HERE, to the last f32 operation, and the sampled ids are reproducible bit for bit (tests/test_gpu_topk_sample.py
// restates it in ~20 lines of NumPy).  Per row the settings are top_k, temperature, topp, minp and the caller's coin (TopkRow):
//   greedy     temperature == 0: the step's greedy first-max id; nothing else of the row is looked at.
//   survivors  kk = min(top_k, vocab).  Logits are compared as floats after l + 0.0f (so -0.0 equals +0.0); the survivors are the first
//              kk entries of the order (logit descending, index ascending) = np.argsort(-l, kind="stable")[:kk].  Logits are finite or
//              -inf; NaN is unspecified.
//   softmax    over the survivors j = 0 .. kk-1 in that order, f32 unless said otherwise: v_j = l_j / temperature,
//              e_j = (float) exp((double) (v_j - v_0)), s = ((0f + e_0) + e_1) + ... strictly sequential, p_j = e_j / s.
//   min-p      for 0 < minp <= 1: keep the prefix of j with p_j >= minp * p_0; at least one entry is kept.
//   top-p      for 0 < topp < 1: inside that prefix the sequential cdf c_n = ((0f + p_0) + ...) + p_{n-1}; n_keep = the smallest n with
//              c_n > topp, the whole prefix if there is none (and with top-p off).
//   draw       r = coin * c_{n_keep}; the token is the survivor at the first j < n_keep with r < c_{j+1}, survivor n_keep - 1 if none.
//   range      1 <= top_k <= 1024 (GL3_E_ARG otherwise); a minp / topp outside its range switches that cut off.
//
// The kernel is a radix SELECT, not a sort of the vocabulary: 1024 threads = 16 wavefronts pull the row four times (0.5-0.6 MB: once from
// HBM or the Infinity Cache, three times from L2) and nothing of [rows][vocab] size is written anywhere.
//   keys     an f32 maps to an order-preserving u32 (tk_key).
//   select   three digit passes (11 + 11 + 10 bits) find the exact 32-bit key T of the kk-th largest element: every wavefront counts the
//            digits of its slab of the row in an LDS histogram of its own (16 x 2048 bins = 128 KB, ds_add), a suffix scan over the bins
//            (tk_find) names the bucket that holds rank kk and how many elements lie above it, and the next pass counts only elements
//            that carry the prefix found so far.  Selecting to the full key before anything is collected keeps the survivor buffer at
//            kk entries even when a bucket holds the whole vocabulary (all logits inside one binade).
//            The top digit is sign + exponent + 2 mantissa bits: a row of ordinary logits puts almost everything into a handful of bins,
//            and a ds_add of 64 lanes to one bin is 64 serial adds.  So pass 0 first counts a prologue (the first 128 quads of every
//            slab, 8192 elements), finds the bucket of rank kk AMONG THOSE — a lower bound for the bucket of rank kk in the whole row,
//            since a subset's kk-th largest is not above the row's — and then skips the ds_add for every digit below it: the bins at and
//            above the bound stay exact, the scan from the top never reaches the others.
//   collect  one more pull: key > T goes straight into the survivor buffer (the slot comes from an LDS counter; WHICH elements get in
//            does not depend on arrival order, and where they stand is settled by the sort).  Of the elements with key == T the
//            kk - count(key > T) LOWEST INDICES are taken, by a slab-ordered prefix count, never by a counter: slabs are contiguous in
//            index order, a wavefront numbers its ties in (iteration, lane, component) = index order with a DPP prefix sum and keeps the
//            indices of its first `need` in LDS; the 16 per-wavefront counts are then scanned and every wavefront copies the share that
//            still fits.  No second pull for the ties.
//   sort     bitonic network in LDS over the power of two at or above kk, on u64 pairs (key << 32 | ~index): descending pairs = key
//            descending, index ascending.  8 KB at kk = 1024.
//   softmax, cuts, draw   exp lane-parallel in double.  The sequential f32 sums (s, then the cdf up to the min-p prefix) run as plain
//            chains on one wavefront / one lane: they are at most 1024 long — 40 in the usual case — and gl3_seqsum.h's exact parallel
//            evaluation needs >= 1024 elements in multiples of 4 (kk == 1024 alone) and gives no prefix values, which the cuts need.
//            The cuts and the pick are lane-parallel minima over the cdf in LDS.
// Settings are read from a per-row device array; no stage takes a per-step scalar, rows are a grid dimension, and a step is ONE launch
// at every row count.  The logits are read through RowLayout (gl3_chunked.h) and never written.  LDS and global atomics are vector
// atomics (ds_add / ds_min); every store is a plain vector store.
// Outputs per row: res {token, n_keep} (greedy: {greedy id, 0}) and, for the parity tap, the kk survivor ids and p_j.
//
// Out of scope, refused by the entries: tp_size > 1 (GL3_E_UNSUPPORTED).  The draft chains and the _dist verification keep taking full
// distributions only: a step of this sampler leaves no row behind that gl3_draft_probs_put / _put_row would file as q.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gl3_chunked.h"
#include "gl3_seqsum.h"      // f2u / u2f, wave_incl_scan_u32, naive_sumsq_lds

namespace gl3 {

constexpr int TK_MAX = 1024;                       // largest top_k
constexpr int TK_THREADS = 1024, TK_WAVES = TK_THREADS / 64;
constexpr int TK_BINS = 2048;                      // bins per wavefront histogram (passes of 11, 11 and 10 bits)
constexpr int TK_PRO_ITERS = 2;                    // pass 0: iterations of every slab counted before the lower bound is taken
constexpr size_t TK_HIST_BYTES = (size_t)TK_WAVES * TK_BINS * 4;
// what lives in the histogram's LDS once the key is selected: pairs u64[TK_MAX], e / p f32[TK_MAX], cdf f32[TK_MAX], ties i32[TK_WAVES][TK_MAX]
constexpr size_t TK_OFF_EP = (size_t)TK_MAX * 8, TK_OFF_CDF = TK_OFF_EP + (size_t)TK_MAX * 4, TK_OFF_TIES = TK_OFF_CDF + (size_t)TK_MAX * 4;
constexpr size_t TK_SMEM = TK_HIST_BYTES;
static_assert(TK_OFF_TIES + (size_t)TK_WAVES * TK_MAX * 4 <= TK_SMEM, "the collect / sort stage reuses the histogram's LDS");
static_assert(2 * TK_THREADS == TK_BINS, "tk_find: two bins per thread");

// A row's settings as the kernel reads them from device memory
struct TopkRow { int top_k; float temperature, topp, minp, coin; };

// order-preserving f32 -> u32 (after l + 0.0f: -0.0 and +0.0 share a key) and back
__device__ __forceinline__ uint32_t tk_key(float l) {
    const uint32_t u = f2u(l + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tk_unkey(uint32_t k) { return u2f((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// Suffix scan over the bins of the 16 histograms: the bin b that holds rank `need` from the top (count(digit > b) < need <= count(digit >= b))
// -> sel[0] = b, sel[1] = count(digit > b).  Thread t owns bins 2047 - 2t and 2046 - 2t, so thread order is descending bin order.  sel is
// left as it was when fewer than `need` elements were counted.  All TK_THREADS threads call it behind a barrier; it ends with one.
__device__ __forceinline__ void tk_find(const uint32_t* hist, uint32_t need, uint32_t* wsum, int* sel, int t) {
    const int b0 = TK_BINS - 1 - 2 * t, b1 = b0 - 1;
    uint32_t c0 = 0, c1 = 0;
#pragma unroll
    for (int w = 0; w < TK_WAVES; ++w) { c0 += hist[w * TK_BINS + b0]; c1 += hist[w * TK_BINS + b1]; }
    const uint32_t incl = wave_incl_scan_u32(c0 + c1);
    if ((t & 63) == 63) wsum[t >> 6] = incl;
    __syncthreads();
    uint32_t above = incl - (c0 + c1);
    for (int w = 0; w < (t >> 6); ++w) above += wsum[w];
    if (above < need && above + c0 >= need) { sel[0] = b0; sel[1] = (int)above; }
    else if (above + c0 < need && above + c0 + c1 >= need) { sel[0] = b1; sel[1] = (int)(above + c0); }
    __syncthreads();
}

// grid = rows, TK_THREADS threads, TK_SMEM bytes of dynamic LDS.  n % 4 == 0 and lay.cc % 16 == 0 (gl3_create), so every quad is one
// aligned float4 that never straddles two rank chunks.  greedy: the step's greedy ids (read for rows at temperature 0 only; may be null
// when no row is greedy).  ids / probs: [rows][TK_MAX].
__global__ __launch_bounds__(TK_THREADS) void topk_sample_kernel(const float* __restrict__ logits, int n, const RowLayout lay, const TopkRow* __restrict__ rows,
                                                                 const int32_t* __restrict__ greedy, int* __restrict__ res, int* __restrict__ ids,
                                                                 float* __restrict__ probs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t tk_smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(tk_smem);
    unsigned long long* pairs = reinterpret_cast<unsigned long long*>(tk_smem);
    float* ep = reinterpret_cast<float*>(tk_smem + TK_OFF_EP);
    float* cdf = reinterpret_cast<float*>(tk_smem + TK_OFF_CDF);
    int* ties = reinterpret_cast<int*>(tk_smem + TK_OFF_TIES);
    __shared__ uint32_t wsum[TK_WAVES];
    __shared__ int sel[2], tie_cnt[TK_WAVES], cnt_gt, m_sh, nk_sh, pick_sh;
    __shared__ float s_sh;
    const int row = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const TopkRow R = rows[row];
    if (R.temperature == 0.f) {
        if (t == 0) { res[2 * row] = greedy[row]; res[2 * row + 1] = 0; }
        return;
    }
    const int kk = min(R.top_k, n);
    // slab of this wavefront: quads [q0, q1), `iters` iterations of 64 quads for every wavefront (the loops and their barriers are uniform)
    const int n4 = n >> 2, q_per = (n4 + TK_WAVES - 1) / TK_WAVES, q0 = min(n4, wave * q_per), q1 = min(n4, q0 + q_per);
    const int iters = (q_per + 63) >> 6;
    // quad `lane` of iteration `it` of the slab (zeros past its end; the caller tests q < q1).  Loaded one iteration ahead of its use,
    // so a wavefront has a load in flight while it counts.
    auto quad = [&](int it) {
        const int q = q0 + it * 64 + lane;
        return q < q1 ? *reinterpret_cast<const float4*>(logits + chunked(row, 4 * q, lay.cc, lay.nrows)) : float4{0.f, 0.f, 0.f, 0.f};
    };

    // ---- select: the key of rank kk, 11 + 11 + 10 bits
    uint32_t prefix = 0, need = (uint32_t)kk, above_total = 0;
    uint32_t* mine = hist + wave * TK_BINS;
    for (int pass = 0; pass < 3; ++pass) {
        const int bits = pass == 2 ? 10 : 11, shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
        for (int i = t; i < TK_WAVES * TK_BINS; i += TK_THREADS) hist[i] = 0u;
        if (t == 0) { sel[0] = 0; sel[1] = 0; }
        __syncthreads();
        uint32_t lb = 0;
        float4 nxt = quad(0);
        for (int it = 0; it < iters; ++it) {
            const float4 v = nxt;
            nxt = quad(it + 1);
            if (pass == 0 && it == TK_PRO_ITERS) {      // the bucket of rank kk among the prologue bounds the row's from below
                __syncthreads();
                tk_find(hist, need, wsum, sel, t);
                lb = (uint32_t)sel[0];
            }
            if (q0 + it * 64 + lane < q1) {
                const uint32_t k[4] = {tk_key(v.x), tk_key(v.y), tk_key(v.z), tk_key(v.w)};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (pass && (k[c] >> (shift + bits)) != prefix) continue;
                    const uint32_t d = (k[c] >> shift) & ((1u << bits) - 1u);
                    if (d >= lb) atomicAdd(&mine[d], 1u);
                }
            }
        }
        __syncthreads();
        if (t == 0) { sel[0] = 0; sel[1] = 0; }      // every read of the prologue's answer lies before the barrier above
        tk_find(hist, need, wsum, sel, t);           // its first barrier orders the reset before the answer is written
        prefix = (prefix << bits) | (uint32_t)sel[0];
        need -= (uint32_t)sel[1];
        above_total += (uint32_t)sel[1];
        __syncthreads();
    }
    const uint32_t T = prefix;                        // `need` >= 1 elements with key == T are still to take, above_total lie above it

    // ---- collect (the histograms are dead: their LDS now holds pairs / ties)
    if (t == 0) cnt_gt = 0;
    __syncthreads();
    int* my_ties = ties + wave * TK_MAX;
    uint32_t wt = 0;                                  // ties this wavefront has met so far (uniform)
    float4 nxt = quad(0);
    for (int it = 0; it < iters; ++it) {
        const int q = q0 + it * 64 + lane;
        const float4 v = nxt;
        nxt = quad(it + 1);
        uint32_t eq = 0;                              // bit c: component c is a tie
        if (q < q1) {
            const uint32_t k[4] = {tk_key(v.x), tk_key(v.y), tk_key(v.z), tk_key(v.w)};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (k[c] > T) {
                    const int slot = atomicAdd(&cnt_gt, 1);
                    if (slot < TK_MAX) pairs[slot] = ((unsigned long long)k[c] << 32) | (uint32_t)~(uint32_t)(4 * q + c);      // slot < above_total < kk by construction
                }
                eq |= (k[c] == T ? 1u : 0u) << c;
            }
        }
        const uint32_t cnt = (uint32_t)__popc(eq);
        const uint32_t incl = wave_incl_scan_u32(cnt);
        uint32_t r = wt + incl - cnt;                 // index order inside a slab: iteration, lane, component
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (eq & (1u << c)) { if (r < need) my_ties[r] = 4 * q + c; ++r; }
        wt += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (lane == 0) tie_cnt[wave] = (int)min(wt, need);
    __syncthreads();
    {
        int base = 0;
        for (int w = 0; w < wave; ++w) base += tie_cnt[w];
        const int take = min(tie_cnt[wave], max((int)need - base, 0));
        for (int i = lane; i < take; i += 64) pairs[above_total + base + i] = ((unsigned long long)T << 32) | (uint32_t)~(uint32_t)my_ties[i];
    }
    int P = 1;
    while (P < kk) P <<= 1;
    if (t >= kk && t < P) pairs[t] = 0ull;            // below every key of a number
    __syncthreads();

    // ---- sort: descending pairs = key descending, index ascending
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int o = t ^ j;
            if (t < P && o > t) {
                const unsigned long long a = pairs[t], b = pairs[o];
                if ((t & k) == 0 ? a < b : a > b) { pairs[t] = b; pairs[o] = a; }
            }
            __syncthreads();
        }

    // ---- softmax over the survivors, cuts, draw
    const float v0 = tk_unkey((uint32_t)(pairs[0] >> 32)) / R.temperature;
    int my_id = 0;
    if (t < kk) {
        const unsigned long long pr = pairs[t];
        my_id = (int)~(uint32_t)pr;
        ep[t] = (float)exp((double)(tk_unkey((uint32_t)(pr >> 32)) / R.temperature - v0));
        ids[(size_t)row * TK_MAX + t] = my_id;
    }
    if (t == 0) { m_sh = kk; }
    __syncthreads();
    if (wave == 0) {
        const float s = naive_sumsq_lds<false>(ep, 0, kk, 0.f);      // ((0f + e_0) + e_1) + ...
        if (lane == 0) s_sh = s;
    }
    __syncthreads();
    float p = 0.f;
    if (t < kk) {
        p = ep[t] / s_sh;
        probs[(size_t)row * TK_MAX + t] = p;
    }
    __syncthreads();                                  // every e is read before a p takes its place
    if (t < kk) ep[t] = p;
    __syncthreads();
    if (R.minp > 0.f && R.minp <= 1.f && t < kk && !(p >= R.minp * ep[0])) atomicMin(&m_sh, t);
    __syncthreads();
    const int m = max(m_sh, 1);
    if (t == 0) {
        float c = 0.f;
        for (int j = 0; j < m; ++j) { c = c + ep[j]; cdf[j] = c; }      // c_{j+1}
        nk_sh = m;
    }
    __syncthreads();
    if (R.topp > 0.f && R.topp < 1.f && t < m && cdf[t] > R.topp) atomicMin(&nk_sh, t + 1);
    __syncthreads();
    const int nk = nk_sh;
    if (t == 0) pick_sh = nk - 1;
    __syncthreads();
    const float r = R.coin * cdf[nk - 1];
    if (t < nk && r < cdf[t]) atomicMin(&pick_sh, t);
    __syncthreads();
    if (t == pick_sh) { res[2 * row] = my_id; res[2 * row + 1] = nk; }
}

}  // namespace gl3
