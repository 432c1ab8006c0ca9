// gl3_sample.hip — temperature / top-p sampling behind the decode step.
//
// Replaces, for the HIP path, Sampler.selectSampler's lambda (J/inference/sampler/Sampler.java:76-123):
//     logits.divideInPlace(temperature); logits.softmaxInPlace();                 FloatTensor.java:203-219
//     CategoricalSampler.sampleToken (J/inference/sampler/CategoricalSampler.java:33-44)   or
//     ToppSampler.sampleToken       (J/inference/sampler/ToppSampler.java:57-160)
// with the reference's arithmetic: f / temperature, max, (float)Math.exp(f - max) in double, the STRICTLY SEQUENTIAL f32 sum
// of all vocab numerators (FloatTensor.sum = reduce(0f, Float::sum)), f / sum, and the sequential f32 cdf of the sampler.
// The 128 k-long sequential sums run on the device with the exact parallel evaluation of gl3_seqsum.h, 4096 elements at a
// time, each chunk starting from the exact running value of the previous one.
//
// The random number stays the CALLER's: `coin` is rng.nextFloat(1f) drawn from the host's RandomGenerator
// (RandomGeneratorFactory.getDefault().create(seed), Sampler.java:84) exactly where the reference draws it — one per sampled
// token — so the stream of random numbers, and with it the sampled ids, are the reference's by construction.
//
// Categorical sampling is entirely on the device (4 bytes come back instead of vocab * 4).  Top-p (r5) too, whenever the answer
// does not hinge on the heap's sift history: the reference's heap selection (ToppSampler.java:118-160) emits the candidates in non-increasing
// VALUE order up to its last three — its one quirk, siftDown(indices, 0, i - 1, ..) leaving the last leaf out of every sift, does not let a
// larger value wait behind a smaller one while the leaf left out has a parent other than the root (the leaf is <= the value its parent had,
// and that value is still in the heap); the leaves at heap positions 2 and 1 hang under the root that was just emitted, so the three
// smallest candidates come out in an order of the heap's own (n0 = 3: the largest, then the two others as they stood; n0 <= 2: sorted) —
// so a truncation point among the first max(n0 - 3, 1) ranks (all of them for n0 <= 2), the renormalised coin and the RANK the coin lands on
// are those of a descending sort, evaluated here with a radix sort + the exact chunked f32 prefix sums; WHICH index stands at a rank shared
// by equal probabilities, and everything about a draw whose cumulative sum does not exceed topp before the heap-ordered tail, is decided by
// the heap's sift history, which no sort order reproduces.  The device path returns the token and a host flag (8 bytes); on a tie at the
// sampled rank (~2 % of the draws on the near-uniform distributions of random-weight test models, rarer on real ones) or a truncation point
// in the tail (a row with a handful of candidates, or a topp so close to the candidates' total that the sum reaches the last three) the
// probabilities are copied out and the reference's heap runs on the host (same sift order, same choice).
//
// One set of kernels serves both entries.  Rows are a grid dimension, and every per-row setting (temperature, topp, coin, mode) is read
// from a small device array (SmpRow, gl3_ctx.h), so no kernel takes a per-step scalar and a step costs the same launches at every row
// count:
//     bsm_scale_max, bsm_exp, bsm_seqsum<false>, bsm_div, bsm_seqsum<true> (categorical pick),
//     btp_keys, 4 x (btp_hist, btp_scan, btp_scatter), btp_pick                      (left out when no row of the step uses top-p)
// A row whose mode does not need a stage returns at once in that stage: greedy rows take the id of the step's own greedy scan
// (pf_argmax_*), categorical rows skip the sort.  The sequential sums keep one workgroup per row (n rows run side by side on n CUs); the
// radix sort is segmented by row (histogram [row][digit][tile], one scan workgroup per row, stable scatter inside the row).  {token, tie}
// of every row come back in one copy of 8 * n bytes; only rows whose flag is set have their probabilities copied out and run through
// the host heap (topp_sample).  The logits are read, never written.
//
// Tensor parallel.  After the logits gather of a batched step every rank holds every row, rank-chunked as [tp][rows][vocab / tp]
// (gl3_chunked.h).  Each rank samples or scores all rows from them redundantly: the same logits and the same coins give the same ids on
// every rank, so nothing is communicated behind the logits gather.  Two kernels read logits and take the layout {chunk width, rows}:
// bsm_scale_max_kernel, whose plain probs rows feed every later sampler stage (tie fallback and parity taps included), and
// score_rows_kernel.  With one rank the chunk width is the vocabulary and the addresses are the plain rows'.  Draft verification
// (verify_runs_kernel) reads plain rows only — the logits and, in its _dist form, the draft distributions: its entries stay one-rank.
//
// Draft distributions.  A target plan keeps q[max_batch][vocab] f32 (gl3_draft_state, allocated on the first put): slot s = the
// distribution ONE drafted token was drawn from, copied on the device from the row a draft PLAN's last gl3_forward_decode_sample left in
// its smp_one.probs (gl3_draft_probs_put; never a top-p row, which is the untruncated softmax).  verify_runs_kernel<true> reads a slot as
// float4 beside the logits quad; nothing else of [rows][vocab] size exists for it.
//
// Draft chain (gl3_forward_decode_chain).  k single-row steps of one plan enqueued back to back: behind each step's sampler (or greedy scan)
// chain_handover_kernel passes the id on to the next step through ctx->dyn and, for a target plan, copies the row into the table itself.
// The sampler's launches are the single-row entry's (sample_launch); only the copy back and the wait happen once per chain.
//
// Batched draft chain (gl3_forward_decode_batch_chain).  The same over static-batched steps: behind each step's batched sampler (or, when
// every row of the step is greedy, its greedy scan) batch_chain_handover_kernel passes every row's id on through the step's own input
// arrays (tokens, positions) and the row's SmpRow, files it in a [k][n] list, and copies the rows that have a slot into the target's table.
// gl3_draft_probs_put_row is that copy as an entry of its own: row `row` of smp_rows.probs into a slot (tools/gl3_spec_batch_run --no-chain).
//
// The two entries are two instances of gl3_sample_state.  gl3_forward_decode_sample is the n = 1 case: 256 workgroups per element-wise
// launch, launched eagerly, its SmpRow riding behind the (token, position) pair in ctx->dyn.  The static-batched entries
// (gl3_forward_decode_batch_sample, gl3_sample_rows) use 64 workgroups per row and replay one hipGraph per (row count, any top-p row).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "gl3_ctx.h"
#include "gl3_chunked.h"      // chunked(), RowLayout: the logits of a tensor-parallel batched step are rank-chunked
#include "gl3_decode_kernels.h"

using namespace gl3;

constexpr int SM_CHUNK = 4096;               // elements per exact sequential-sum chunk

// aux row layout: `blocks` block maxima, the total, nchunks chunk ends.  blocks = workgroups per row of the element-wise launches
// (gl3_sample_state::blocks, at most 256: bsm_exp reads one maximum per thread); the maximum does not depend on how rows are split.
// The one sampler kernel that reads the logits (lay: where element i of a row is, gl3_chunked.h); everything behind it works on probs, plain rows.
__global__ __launch_bounds__(256) void bsm_scale_max_kernel(const float* __restrict__ logits, int n, const RowLayout lay, const SmpRow* __restrict__ rows, const int32_t* __restrict__ greedy,
                                                            float* __restrict__ probs, float* __restrict__ aux, int aux_stride, int* __restrict__ res, int* __restrict__ n0) {
    __shared__ float red[4];
    const int row = blockIdx.y;
    const SmpRow R = rows[row];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        n0[row] = 0;
        if (R.mode == SMP_GREEDY) { res[2 * row] = greedy[row]; res[2 * row + 1] = 0; }
    }
    if (R.mode == SMP_GREEDY) return;
    float* p = probs + (size_t)row * n;
    float mx = -INFINITY;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float v = logits[chunked(row, i, lay.cc, lay.nrows)] / R.temperature;                         // divideInPlace(temperature)
        p[i] = v;
        mx = fmaxf(mx, v);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) aux[(size_t)row * aux_stride + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void bsm_exp_kernel(float* __restrict__ probs, int n, const SmpRow* __restrict__ rows, const float* __restrict__ aux, int aux_stride, int blocks) {
    __shared__ float red[4];
    const int row = blockIdx.y;
    if (rows[row].mode == SMP_GREEDY) return;
    float* p = probs + (size_t)row * n;
    const float* blockmax = aux + (size_t)row * aux_stride;
    float mx = threadIdx.x < blocks ? blockmax[threadIdx.x] : -INFINITY;
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) p[i] = (float)exp((double)(p[i] - mx));   // (float) Math.exp(f - maxVal)
}

// Strictly sequential f32 sum of a row's p[0..n) (all >= 0), one workgroup per row: chunks of SM_CHUNK through LDS, exact parallel
// evaluation per chunk (gl3_seqsum.h) continued from the exact running value.  chunk_end[c] = running sum after chunk c (the cdf at
// the chunk boundaries).  PICK = false: every non-greedy row, total and chunk ends of the numerators; PICK = true: categorical rows
// only, res[row] = {first index whose cdf exceeds the row's coin (CategoricalSampler), 0}.
template <bool PICK>
__global__ __launch_bounds__(256) void bsm_seqsum_kernel(const float* __restrict__ probs, int n, const SmpRow* __restrict__ rows, float* __restrict__ aux, int aux_stride,
                                                         int blocks, int* __restrict__ res) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* xf = reinterpret_cast<float*>(smem);                      // [SM_CHUNK + 32]
    uint8_t* scratch = smem + (size_t)(SM_CHUNK + 32) * 4;
    __shared__ float run_s;
    __shared__ int hit_s;
    const int row = blockIdx.x;
    const SmpRow R = rows[row];
    if (PICK ? R.mode != SMP_CATEGORICAL : R.mode == SMP_GREEDY) return;
    const float* p = probs + (size_t)row * n;
    float* total = aux + (size_t)row * aux_stride + blocks;
    float* chunk_end = total + 1;
    const float coin = R.coin;
    int* picked = res + 2 * row;
    const int t = threadIdx.x;
    if (t == 0) { run_s = 0.f; hit_s = -1; if (PICK) picked[1] = 0; }
    __syncthreads();
    const int nchunks = (n + SM_CHUNK - 1) / SM_CHUNK;
    for (int c = 0; c < nchunks; ++c) {
        const int base = c * SM_CHUNK, len = min(SM_CHUNK, n - base);
        for (int i = t; i < SM_CHUNK + 32; i += 256) xf[i] = i < len ? p[base + i] : 0.f;
        __syncthreads();
        float run = run_s;
        const int n4 = len & ~3;
        if (n4 >= 1024) {
            BlockBarrier bb;
            run = exact_seqsum_lds<false>(xf, n4, scratch, t, bb, run);
            if (n4 < len && t < 64) run = naive_sumsq_lds<false>(xf, n4, len, run);      // at most 3 trailing elements
        } else if (t < 64) {
            run = naive_sumsq_lds<false>(xf, 0, len, run);
        }
        __syncthreads();
        if (t == 0) {
            if (PICK && hit_s < 0 && coin < run) hit_s = c;           // the cdf is non-decreasing: the first chunk whose end exceeds coin
            run_s = run;
            chunk_end[c] = run;
        }
        __syncthreads();
        if (PICK && hit_s == c) {
            // cdf += p[i]; if (coin < cdf) return i   (CategoricalSampler.java:37-42), continued inside the chunk from its exact start
            if (t == 0) {
                float cdf = c ? chunk_end[c - 1] : 0.f;
                int idx = -1;
                for (int i = 0; i < len; ++i) { cdf = cdf + xf[i]; if (coin < cdf) { idx = base + i; break; } }
                picked[0] = idx >= 0 ? idx : base + len - 1;
            }
            break;
        }
    }
    __syncthreads();
    if (t == 0) {
        if (!PICK) *total = run_s;
        if (PICK && hit_s < 0) picked[0] = n - 1;                     // "in case of rounding errors"
    }
}

__global__ __launch_bounds__(256) void bsm_div_kernel(float* __restrict__ probs, int n, const SmpRow* __restrict__ rows, const float* __restrict__ aux, int aux_stride, int blocks) {
    const int row = blockIdx.y;
    if (rows[row].mode == SMP_GREEDY) return;
    float* p = probs + (size_t)row * n;
    const float s = aux[(size_t)row * aux_stride + blocks];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) p[i] = p[i] / s;     // divideInPlace(sum)
}

// ToppSampler (J/inference/sampler/ToppSampler.java:57-160) on host probabilities — same cutoff, same heap build / sift order,
// same cumulative f32 sums, so the same index also when probabilities tie.
static void sift_down(int* array, int from, int n, const float* v) {
    auto cmp = [&](int a, int b) {          // Comparator.comparingDouble(getFloat).reversed(): negative when a's value is LARGER
        const double da = v[a], db = v[b];
        return db < da ? -1 : db > da ? 1 : 0;
    };
    int prev = from, next;
    while ((next = 2 * prev + 1) < n) {
        const int r = 2 * prev + 2;
        if (r < n && cmp(array[r], array[next]) < 0) next = r;
        if (cmp(array[next], array[prev]) < 0) { std::swap(array[prev], array[next]); prev = next; }
        else break;
    }
}

static int topp_sample(const float* p, int n, float topp, float coin, std::vector<int>& indices) {
    indices.resize(n);
    int head = 0, tail = n - 1;
    const float cutoff = (1.0f - topp) / (float)(n - 1);
    for (int i = 0; i < n; ++i) {
        if (p[i] >= cutoff) indices[head++] = i;
        else indices[tail--] = i;
    }
    const int n0 = head;
    int* idx = indices.data();
    for (int i = n0 / 2 - 1; i >= 0; --i) sift_down(idx, i, n0, p);
    float cumulative = 0.0f;
    int last = 0;
    for (int i = n0 - 1; i >= 0; --i) {
        std::swap(idx[0], idx[i]);
        cumulative += p[idx[i]];
        if (cumulative > topp) { last = i; break; }
        sift_down(idx, 0, i - 1, p);
    }
    const float r = coin * cumulative;
    float cdf = 0.0f;
    for (int i = n0 - 1; i >= last; --i) {
        cdf += p[idx[i]];
        if (r < cdf) return idx[i];
    }
    return idx[last];
}

// ------------------------------------------------------------------------------------------------ top-p on the device
// Keys: candidates (p >= cutoff, ToppSampler.java:74-81) get ~bits(p) (positive floats order like their bit patterns, so ascending keys
// = descending probabilities), everything else the maximal key; a stable LSD radix sort (4 x 8 bits) of (key, index) pairs, segmented by
// row, puts the n0 candidates first in descending order.  A row's segment of `sort`: ka[n] ia[n] kb[n] ib[n] hist[256 nb].
constexpr int RS_THREADS = 256, RS_PER = 4, RS_TILE = RS_THREADS * RS_PER;
struct BtpSeg {
    uint32_t *ka, *kb;
    int *ia, *ib, *hist;
    __device__ BtpSeg(uint32_t* sort, size_t stride, int row, int n) {
        ka = sort + (size_t)row * stride;
        ia = reinterpret_cast<int*>(ka + n);
        kb = reinterpret_cast<uint32_t*>(ia + n);
        ib = reinterpret_cast<int*>(kb + n);
        hist = ib + n;
    }
};

__global__ __launch_bounds__(RS_THREADS) void btp_keys_kernel(const float* __restrict__ probs, int n, const SmpRow* __restrict__ rows, uint32_t* __restrict__ sort, size_t stride,
                                                               int* __restrict__ n0) {
    __shared__ int cnt_s;
    const int row = blockIdx.y;
    const SmpRow R = rows[row];
    if (R.mode != SMP_TOPP) return;
    const float cutoff = (1.0f - R.topp) / (float)(n - 1);            // ToppSampler.java:73
    const float* p = probs + (size_t)row * n;
    const BtpSeg S(sort, stride, row, n);
    if (threadIdx.x == 0) cnt_s = 0;
    __syncthreads();
    int c = 0;
    for (int i = blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += gridDim.x * RS_THREADS) {
        const float v = p[i];
        const bool cand = v >= cutoff;
        S.ka[i] = cand ? ~__builtin_bit_cast(uint32_t, v) : 0xFFFFFFFFu;
        S.ia[i] = i;
        c += cand ? 1 : 0;
    }
    atomicAdd(&cnt_s, c);
    __syncthreads();
    if (threadIdx.x == 0 && cnt_s) atomicAdd(n0 + row, cnt_s);
}

// hist[row][d * nblocks + b] = elements of tile b of the row whose digit is d.  pass = 0..3: odd passes read (kb, ib).
__global__ __launch_bounds__(RS_THREADS) void btp_hist_kernel(const SmpRow* __restrict__ rows, uint32_t* __restrict__ sort, size_t stride, int n, int pass, int nblocks) {
    __shared__ int h[256];
    const int row = blockIdx.y;
    if (rows[row].mode != SMP_TOPP) return;
    const BtpSeg S(sort, stride, row, n);
    const uint32_t* keys = pass & 1 ? S.kb : S.ka;
    const int shift = 8 * pass;
    h[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_PER; ++r) {
        const int e = blockIdx.x * RS_TILE + r * RS_THREADS + threadIdx.x;
        if (e < n) atomicAdd(&h[(keys[e] >> shift) & 255u], 1);
    }
    __syncthreads();
    S.hist[threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

// exclusive prefix over a row's histogram in (digit, tile) order, in place; one workgroup of 1024 threads per row
__global__ __launch_bounds__(1024) void btp_scan_kernel(const SmpRow* __restrict__ rows, uint32_t* __restrict__ sort, size_t stride, int n, int total) {
    __shared__ int part[1024];
    const int row = blockIdx.x;
    if (rows[row].mode != SMP_TOPP) return;
    int* hist = BtpSeg(sort, stride, row, n).hist;
    const int t = threadIdx.x, per = (total + 1023) / 1024, lo = min(total, t * per), hi = min(total, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += hist[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = lo; i < hi; ++i) { const int v = hist[i]; hist[i] = run; run += v; }
}

// stable scatter of tile blockIdx.x of row blockIdx.y: element order inside a tile is (round, wavefront, lane) = ascending index
__global__ __launch_bounds__(RS_THREADS) void btp_scatter_kernel(const SmpRow* __restrict__ rows, uint32_t* __restrict__ sort, size_t stride, int n, int pass, int nblocks) {
    __shared__ int base[256];                  // next output slot of digit d for this tile
    __shared__ int wcnt[4][256];               // per wavefront: elements of digit d in the current round
    const int row = blockIdx.y;
    if (rows[row].mode != SMP_TOPP) return;
    const BtpSeg S(sort, stride, row, n);
    const uint32_t* kin = pass & 1 ? S.kb : S.ka;
    const int* iin = pass & 1 ? S.ib : S.ia;
    uint32_t* kout = pass & 1 ? S.ka : S.kb;
    int* iout = pass & 1 ? S.ia : S.ib;
    const int shift = 8 * pass;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    base[t] = S.hist[t * nblocks + blockIdx.x];
#pragma unroll
    for (int r = 0; r < RS_PER; ++r) {
#pragma unroll
        for (int w = 0; w < 4; ++w) wcnt[w][t] = 0;
        __syncthreads();
        const int e = blockIdx.x * RS_TILE + r * RS_THREADS + t;
        const bool valid = e < n;
        const uint32_t key = valid ? kin[e] : 0u;
        const int id = valid ? iin[e] : 0;
        const uint32_t d = (key >> shift) & 255u;
        // lanes of my wavefront holding the same digit (8 ballots); invalid lanes match nobody
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long vote = __ballot(valid && ((d >> b) & 1u));
            same &= ((d >> b) & 1u) ? vote : ~vote;
        }
        const int before = __popcll(same & ((1ull << lane) - 1ull));
        if (valid && before == 0) wcnt[wave][d] = __popcll(same);
        __syncthreads();
        if (valid) {
            int off = base[d] + before;
            for (int w = 0; w < wave; ++w) off += wcnt[w][d];
            if (off >= 0 && off < n) {         // a row-relative slot by construction; never write outside the row's segment
                kout[off] = key;
                iout[off] = id;
            }
        }
        __syncthreads();
        base[t] += wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
        __syncthreads();
    }
}

// ToppSampler.processTopP :118-160 on a row's sorted candidates sv[0 .. n0) (sv[r] = probability at rank r, descending), one workgroup
// per row:
//   cumulativeProb += value (f32, in order) until it EXCEEDS topp -> last rank (rank n0 - 1 if it never does);
//   r = coin * cumulativeProb;  cdf += value from rank 0: the first rank with r < cdf, bounded by the last rank.
// The two strictly sequential prefix scans run 4096 ranks at a time with the exact parallel sum (gl3_seqsum.h) and walk only the
// chunk in which the threshold falls.  res[row] = {index at the chosen rank, 1 if another candidate has the same probability or the sum
// did not exceed topp within the ranks the reference emits in sorted order (all but its last three, see the head of this file) — then the
// reference's heap order, not this sort order, names the token: the host re-runs it}.
__global__ __launch_bounds__(256) void btp_pick_kernel(const SmpRow* __restrict__ rows, uint32_t* __restrict__ sort, size_t stride, int n, const int* __restrict__ n0p,
                                                       int* __restrict__ res) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* xf = reinterpret_cast<float*>(smem);                      // [SM_CHUNK + 32]
    uint8_t* scratch = smem + (size_t)(SM_CHUNK + 32) * 4;
    __shared__ float run_s, thr_s, cum_s;
    __shared__ int rank_s, last_s;
    const int row = blockIdx.x;
    const SmpRow R = rows[row];
    if (R.mode != SMP_TOPP) return;
    const BtpSeg S(sort, stride, row, n);
    const uint32_t* skeys = S.ka;                                    // 4 passes: the sorted pairs are back in (ka, ia)
    const int* sidx = S.ia;
    int* out = res + 2 * row;
    const float topp = R.topp, coin = R.coin;
    const int t = threadIdx.x;
    const int n0 = min(n0p[row], n);
    if (n0 <= 0) { if (t == 0) { out[0] = 0; out[1] = 1; } return; }      // no candidate (cannot happen for a normalised row): let the host decide
    if (t == 0) { thr_s = topp; last_s = n0 - 1; cum_s = 0.f; }
    const int sorted = n0 <= 2 ? n0 : max(n0 - 3, 1);                // ranks the reference's heap emits in descending order
    bool heap_tail = false;                                          // thread 0: the truncation point is not among them
    for (int phase = 0; phase < 2; ++phase) {
        if (t == 0) { run_s = 0.f; rank_s = -1; }
        __syncthreads();
        const float thr = thr_s;
        const int limit = phase == 0 ? n0 : last_s + 1;              // phase 1 never looks past the truncation point
        for (int base = 0; base < limit; base += SM_CHUNK) {
            const int len = min(SM_CHUNK, limit - base);
            for (int i = t; i < SM_CHUNK + 32; i += 256) xf[i] = i < len ? __builtin_bit_cast(float, ~skeys[base + i]) : 0.f;
            __syncthreads();
            const float start = run_s;
            float run = start;
            const int n4 = len & ~3;
            if (n4 >= 1024) {
                BlockBarrier bb;
                run = exact_seqsum_lds<false>(xf, n4, scratch, t, bb, run);
                if (n4 < len && t < 64) run = naive_sumsq_lds<false>(xf, n4, len, run);
            } else if (t < 64) {
                run = naive_sumsq_lds<false>(xf, 0, len, run);
            }
            __syncthreads();
            if (t == 0) {
                if (thr < run) {                                       // the prefix is non-decreasing: the threshold falls in this chunk
                    float cdf = start;
                    int hit = len - 1;
                    for (int i = 0; i < len; ++i) { cdf = cdf + xf[i]; if (thr < cdf) { hit = i; break; } }
                    rank_s = base + hit;
                    run = cdf;
                }
                run_s = run;
            }
            __syncthreads();
            if (rank_s >= 0) break;
        }
        if (t == 0) {
            if (phase == 0) {
                heap_tail = rank_s < 0 || rank_s >= sorted;            // the sum reaches the ranks whose order is the heap's own: the host decides
                if (rank_s >= 0) last_s = rank_s;                      // cumulativeProb > topp at this rank (its value included)
                cum_s = run_s;                                         // else: every candidate, lastIndex = 0 in the reference
                thr_s = coin * cum_s;                                  // rng.nextFloat(1f) * cumulativeProb
            } else if (rank_s < 0) rank_s = last_s;                    // "in case of rounding errors"
        }
        __syncthreads();
    }
    if (t == 0) {
        const int r = rank_s;
        const uint32_t k = skeys[r];
        const bool tie = (r > 0 && skeys[r - 1] == k) || (r + 1 < n0 && skeys[r + 1] == k);
        out[0] = sidx[r];
        out[1] = tie || heap_tail ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ token scores
// gl3_forward_batch_score / gl3_score_rows: the probability softmaxInPlace(logits / temperature) gives ONE known token per row (the next
// token of a text, a drafted token), FloatTensor.java:203-219 with the arithmetic of the sampler above — but nothing of a row is kept
// except four floats.  One launch, one workgroup per row, rows a grid dimension, the row's settings read from device memory (ScoreRow):
//   pass 1  the row's maximum.  Found by a first pass over the row INSIDE this kernel rather than by block maxima in a launch of its own:
//           the workgroup that sums a row sequentially has to stream the whole row anyway, so a separate launch would add a launch gap
//           and an O(rows * blocks) buffer to save one read that the second pass then finds in L2 / the Infinity Cache; with many rows
//           (a perplexity chunk) every CU has a row of its own and the machine is as busy as block maxima would make it.  Division by a
//           positive temperature is monotone under round-to-nearest, so max_i (l[i] / T) = (max_i l[i]) / T: one division.
//   pass 2  SM_CHUNK numerators (float) exp((double)(l[i] / T - max)) at a time into LDS, then the strictly sequential f32 sum of the chunk
//           continued from the exact running value, with bsm_seqsum_kernel's split: exact_seqsum_lds for >= 1024 elements (multiple of 4),
//           the naive chain for a shorter chunk and for up to 3 trailing elements.  The numerator of the target is picked up from LDS in
//           the chunk that holds it.
// No [rows][vocab] intermediate exists: device memory grows by 8 + 16 bytes per row.  The logits are read, never written.
// n % 4 == 0 (gl3_create: vocab is a multiple of 16), so rows are 16-byte aligned and every global / LDS access is a float4.
// lay: where element i of a row is (gl3_chunked.h).  A chunk width is a multiple of 16, so a quad never straddles two rank chunks; an SM_CHUNK
// piece may, and a chunk boundary may fall inside a piece: every quad is addressed on its own.
__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ logits, int n, const RowLayout lay, const ScoreRow* __restrict__ rows,
                                                         gl3_token_score* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* xf = reinterpret_cast<float*>(smem);                      // [SM_CHUNK + 32]
    uint8_t* scratch = smem + (size_t)(SM_CHUNK + 32) * 4;
    float* sh = reinterpret_cast<float*>(scratch + ss_scratch_bytes(SM_CHUNK));      // [0..3] wavefront maxima, [4] running sum, [5] target numerator
    const int row = blockIdx.x;
    const ScoreRow R = rows[row];
    const float T = R.temperature;
    auto quad = [&](int i) { return *reinterpret_cast<const float4*>(logits + chunked(row, i, lay.cc, lay.nrows)); };      // elements i .. i + 3, i % 4 == 0
    const int t = threadIdx.x;
    float mx = -INFINITY;
    for (int i = t; i < (n >> 2); i += 256) {
        const float4 v = quad(4 * i);
        mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    mx = wave_max(mx);
    if ((t & 63) == 0) sh[t >> 6] = mx;
    if (t == 0) { sh[4] = 0.f; sh[5] = 0.f; }
    __syncthreads();
    mx = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])) / T;      // divideInPlace(temperature), then max
    const int nchunks = (n + SM_CHUNK - 1) / SM_CHUNK;
    for (int c = 0; c < nchunks; ++c) {
        const int base = c * SM_CHUNK, len = min(SM_CHUNK, n - base);
        for (int i = 4 * t; i < SM_CHUNK + 32; i += 1024) {
            float4 e = {0.f, 0.f, 0.f, 0.f};                          // zero padding behind the chunk (exact_seqsum_lds reads it)
            if (i < len) {
                const float4 v = quad(base + i);
                e.x = (float)exp((double)(v.x / T - mx));            // (float) Math.exp(f - maxVal)
                e.y = (float)exp((double)(v.y / T - mx));
                e.z = (float)exp((double)(v.z / T - mx));
                e.w = (float)exp((double)(v.w / T - mx));
            }
            *reinterpret_cast<float4*>(xf + i) = e;
        }
        __syncthreads();
        float run = sh[4];
        const int n4 = len & ~3;
        if (n4 >= 1024) {
            BlockBarrier bb;
            run = exact_seqsum_lds<false>(xf, n4, scratch, t, bb, run);
            if (n4 < len && t < 64) run = naive_sumsq_lds<false>(xf, n4, len, run);      // at most 3 trailing elements
        } else if (t < 64) {
            run = naive_sumsq_lds<false>(xf, 0, len, run);
        }
        __syncthreads();
        if (t == 0) {
            sh[4] = run;
            if (R.target >= base && R.target < base + len) sh[5] = xf[R.target - base];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float sum = sh[4];
        const float4 o = {sh[5] / sum, logits[chunked(row, R.target, lay.cc, lay.nrows)] / T, mx, sum};      // softmaxInPlace(v)[target], v[target], max, sum
        *reinterpret_cast<float4*>(out + row) = o;
    }
}

// ------------------------------------------------------------------------------------------------ draft verification
// gl3_forward_batch_verify / gl3_verify_rows: how many drafted tokens of a run stand and which token follows them.  One launch, one
// workgroup per RUN (runs are the grid), the run's and its rows' settings read from device memory (VerifyRun, VerifyRow); 8 bytes per run
// come back.  In a run of m rows, row i predicts the token after its own, so its draft is d = the token of row i + 1; the last row has none.
//   greedy run (temperature 0)  one thread walks the step's own greedy ids (pf_argmax_*): a = the leading rows whose greedy id equals
//                               their draft, token = the greedy id of row a.  Nothing of the logits is read.
//   sampled run                 rows in order, stopping at the first rejection, so a row behind it is never exponentiated.  Per row the two
//                               passes of score_rows_kernel — the maximum, then SM_CHUNK numerators (float) exp((double) (l / T - max)) at a
//                               time through LDS into the strictly sequential f32 sum — give p[d] = e[d] / sum, bit for bit
//                               gl3_token_score.prob; the row accepts iff its accept coin < p[d].  The row a that rejects (or row m - 1,
//                               which has no draft) then emits: q = e / sum with q[d] = 0f, chunk by chunk into the sequential sum S' whose
//                               value after every chunk stays in LDS; r = emit coin * S' (no draft: q = p and r = the coin, which is
//                               CategoricalSampler, so the walk stops at the first chunk whose end exceeds the coin); the first chunk whose
//                               end exceeds r is recomputed and one thread walks its cdf from the chunk's exact start to the first j
//                               with r < cdf.  q[d] = 0 leaves the cdf at d where it was at d - 1, so d is never that j.  No chunk end above
//                               r: the largest index other than d ("in case of rounding errors", CategoricalSampler.java:43).
//   sampled run, a row whose    (gl3_forward_batch_verify_dist / gl3_verify_rows_dist, DIST = true, VerifyRow::q >= 0; a row with q = -1 is
//   draft was drawn from q      decided as above, bit for bit.)  p[d] as above; the row accepts iff accept coin * q[d] < p[d] — one f32
//                               product, no division: min(1, p[d] / q[d]) without the quotient, and q[d] == 0 accepts iff p[d] > 0.  The
//                               row that rejects emits from the residual r[j] = fmaxf(e[j] / sum - q[j], 0f), the q quad read beside the
//                               logits quad: S', the chunk ends and the walk of the hit chunk as above with r = emit coin * S'.  A
//                               rejection implies q[d] >= p[d], so r[d] == 0 and d cannot come back; nothing special-cases it.  No chunk
//                               end above r: S' == 0 (p <= q everywhere) -> the row's greedy id from the step's own greedy scan; S' > 0
//                               (the product rounded up to S') -> the largest j with r[j] > 0, which every thread tracks while it
//                               fills the chunks.  Lossless for a d drawn from q:
//                               P(first emitted = x) = q(x) min(1, p(x) / q(x)) + (1 - sum min(p, q)) max(p(x) - q(x), 0) / sum max(p - q, 0)
//                               = min(p(x), q(x)) + max(p(x) - q(x), 0) = p(x), since 1 - sum min(p, q) = sum max(p - q, 0).
// Numerators are recomputed where they are needed a second time (one row and one chunk per run) instead of kept: no [rows][vocab] buffer
// exists beside the logits (and the draft table), which are read, never written.  n % 4 == 0 as in score_rows_kernel.
// LDS, all dynamic (verify_smem): xf [SM_CHUNK + 32], the scratch of exact_seqsum_lds, sh [8] ([0..3] wavefront maxima, [4] running sum,
// [5] numerator of the draft, [6] accept flag / hit chunk; DIST: sh [12], [8] the largest index with a positive residual), cend [nchunks].
// The strictly sequential f32 sum of the LDS chunk xf[0 .. len) (all >= 0, zeros behind it up to SM_CHUNK + 32) continued from the exact
// running value `run`: the exact parallel evaluation (gl3_seqsum.h) for >= 1024 elements (a multiple of 4), the naive chain for a
// shorter chunk and for up to 3 trailing elements.  All 256 threads call it between two barriers; thread 0 holds the result.  (The split of
// bsm_seqsum_kernel, btp_pick_kernel and score_rows_kernel, which keep their own copies.)
__device__ __forceinline__ float chunk_seqsum(const float* xf, int len, uint8_t* scratch, int t, float run) {
    const int n4 = len & ~3;
    if (n4 >= 1024) {
        BlockBarrier bb;
        run = exact_seqsum_lds<false>(xf, n4, scratch, t, bb, run);
        if (n4 < len && t < 64) run = naive_sumsq_lds<false>(xf, n4, len, run);
    } else if (t < 64) {
        run = naive_sumsq_lds<false>(xf, 0, len, run);
    }
    return run;
}

template <bool EMIT>
__device__ __forceinline__ void verify_fill_chunk(float* xf, const float4* lg4, int base, int len, float T, float mx, float sum, int d, int t) {
    for (int i = 4 * t; i < SM_CHUNK + 32; i += 1024) {
        float4 e = {0.f, 0.f, 0.f, 0.f};                              // zero padding behind the chunk (exact_seqsum_lds reads it)
        if (i < len) {
            const float4 v = lg4[(base + i) >> 2];
            e.x = (float)exp((double)(v.x / T - mx));                // (float) Math.exp(f - maxVal)
            e.y = (float)exp((double)(v.y / T - mx));
            e.z = (float)exp((double)(v.z / T - mx));
            e.w = (float)exp((double)(v.w / T - mx));
            if (EMIT) {
                const int j = base + i;
                e.x = j == d ? 0.f : e.x / sum;                       // divideInPlace(sum); the rejected draft cannot be drawn again
                e.y = j + 1 == d ? 0.f : e.y / sum;
                e.z = j + 2 == d ? 0.f : e.z / sum;
                e.w = j + 3 == d ? 0.f : e.w / sum;
            }
        }
        *reinterpret_cast<float4*>(xf + i) = e;
    }
}

// The residual of a row whose draft was drawn from q: r[j] = fmaxf(e[j] / sum - q[j], 0f), the q quad read beside the logits quad (q4: the
// slot's row, 16-byte aligned as the logits row is).  Returns the largest index of the chunk this thread gave a positive r, or -1.
__device__ __forceinline__ int verify_fill_chunk_dist(float* xf, const float4* lg4, const float4* q4, int base, int len, float T, float mx, float sum, int t) {
    int last = -1;
    for (int i = 4 * t; i < SM_CHUNK + 32; i += 1024) {
        float4 e = {0.f, 0.f, 0.f, 0.f};                              // zero padding behind the chunk (exact_seqsum_lds reads it)
        if (i < len) {
            const float4 v = lg4[(base + i) >> 2];
            const float4 q = q4[(base + i) >> 2];
            e.x = fmaxf((float)exp((double)(v.x / T - mx)) / sum - q.x, 0.f);      // max(p - q, 0): p exactly as the accept test saw it
            e.y = fmaxf((float)exp((double)(v.y / T - mx)) / sum - q.y, 0.f);
            e.z = fmaxf((float)exp((double)(v.z / T - mx)) / sum - q.z, 0.f);
            e.w = fmaxf((float)exp((double)(v.w / T - mx)) / sum - q.w, 0.f);
            const int j = base + i;
            last = e.w > 0.f ? j + 3 : e.z > 0.f ? j + 2 : e.y > 0.f ? j + 1 : e.x > 0.f ? j : last;
        }
        *reinterpret_cast<float4*>(xf + i) = e;
    }
    return last;
}

// sh words in front of cend.  DIST adds [8] (an int) the largest index with a positive residual.
constexpr int VERIFY_SH = 8, VERIFY_SH_DIST = 12;
constexpr size_t verify_smem(int nchunks, bool dist) {
    return (size_t)(SM_CHUNK + 32) * 4 + ss_scratch_bytes(SM_CHUNK) + (size_t)(dist ? VERIFY_SH_DIST : VERIFY_SH) * 4 + (size_t)nchunks * 4;
}

// DIST = false: gl3_forward_batch_verify / gl3_verify_rows, every draft a fixed token (qtab is not looked at).  DIST = true: the _dist
// entries; a row whose VerifyRow::q names a slot of qtab ([slots][n]) is decided against that distribution, every other row as before.
template <bool DIST>
__global__ __launch_bounds__(256) void verify_runs_kernel(const float* __restrict__ logits, int n, const VerifyRun* __restrict__ runs, const VerifyRow* __restrict__ rows,
                                                          const int32_t* __restrict__ greedy, gl3_verify_result* __restrict__ out, const float* __restrict__ qtab) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* xf = reinterpret_cast<float*>(smem);                      // [SM_CHUNK + 32]
    uint8_t* scratch = smem + (size_t)(SM_CHUNK + 32) * 4;
    float* sh = reinterpret_cast<float*>(scratch + ss_scratch_bytes(SM_CHUNK));
    float* cend = sh + (DIST ? VERIFY_SH_DIST : VERIFY_SH);          // [nchunks] S' after every chunk of the emitting row
    const VerifyRun R = runs[blockIdx.x];
    const int t = threadIdx.x;
    if (R.temperature == 0.f) {
        if (t == 0) {
            int a = 0;
            while (a + 1 < R.rows && greedy[R.row0 + a] == rows[R.row0 + a + 1].token) ++a;
            out[blockIdx.x] = gl3_verify_result{a, greedy[R.row0 + a]};
        }
        return;
    }
    const float T = R.temperature;
    const int nchunks = (n + SM_CHUNK - 1) / SM_CHUNK;
    for (int a = 0; a < R.rows; ++a) {
        const int row = R.row0 + a;
        const int d = a + 1 < R.rows ? rows[row + 1].token : -1;
        const float4* lg4 = reinterpret_cast<const float4*>(logits + (size_t)row * n);
        const float4* q4 = nullptr;                                   // DIST: the distribution d was drawn from; null = a fixed token
        if constexpr (DIST) {
            const int qs = d >= 0 ? rows[row].q : -1;
            if (qs >= 0) q4 = reinterpret_cast<const float4*>(qtab + (size_t)qs * n);
        }
        float mx = -INFINITY;
        for (int i = t; i < (n >> 2); i += 256) {
            const float4 v = lg4[i];
            mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
        }
        mx = wave_max(mx);
        if ((t & 63) == 0) sh[t >> 6] = mx;
        if (t == 0) { sh[4] = 0.f; sh[5] = 0.f; }
        __syncthreads();
        mx = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])) / T;      // divideInPlace(temperature), then max (score_rows_kernel)
        for (int c = 0; c < nchunks; ++c) {
            const int base = c * SM_CHUNK, len = min(SM_CHUNK, n - base);
            verify_fill_chunk<false>(xf, lg4, base, len, T, mx, 0.f, -1, t);
            __syncthreads();
            const float run = chunk_seqsum(xf, len, scratch, t, sh[4]);
            __syncthreads();
            if (t == 0) {
                sh[4] = run;
                if (d >= base && d < base + len) sh[5] = xf[d - base];
            }
            __syncthreads();
        }
        const float sum = sh[4];
        if (DIST && q4) {
            if (t == 0) sh[6] = rows[row].accept * reinterpret_cast<const float*>(q4)[d] < sh[5] / sum ? 1.f : 0.f;      // accept iff coin * q[d] < p[d], strictly
        } else {
            if (t == 0) sh[6] = d >= 0 && rows[row].accept < sh[5] / sum ? 1.f : 0.f;      // accept iff coin < p[d], strictly
        }
        __syncthreads();
        if (sh[6] != 0.f) continue;      // every thread read `sum` and the flag; the next row writes sh[4..6] behind barriers of its own
        // ---- row a emits
        const float coin = rows[row].emit;
        if (t == 0) sh[4] = 0.f;
        __syncthreads();
        int walked = 0;
        int last = -1;                                                // DIST: the largest index this thread gave a positive residual
        for (int c = 0; c < nchunks; ++c) {
            const int base = c * SM_CHUNK, len = min(SM_CHUNK, n - base);
            if (DIST && q4) last = max(last, verify_fill_chunk_dist(xf, lg4, q4, base, len, T, mx, sum, t));
            else verify_fill_chunk<true>(xf, lg4, base, len, T, mx, sum, d, t);
            __syncthreads();
            const float run = chunk_seqsum(xf, len, scratch, t, sh[4]);
            __syncthreads();
            if (t == 0) { sh[4] = run; cend[c] = run; }
            __syncthreads();
            walked = c + 1;
            if (d < 0 && coin < sh[4]) break;                          // no draft: the cdf of p itself, the first chunk whose end exceeds the coin
        }
        const float r = d >= 0 ? coin * sh[4] : coin;                  // coin * S'
        if (t == 0) {
            int hit = -1;
            for (int c = 0; c < walked; ++c) if (r < cend[c]) { hit = c; break; }      // the cdf is non-decreasing
            sh[6] = (float)hit;
        }
        __syncthreads();
        const int hit = (int)sh[6];
        int token = d == n - 1 ? n - 2 : n - 1;                        // no j with r < cdf_j: the largest index other than d
        if (DIST && q4 && hit < 0) {
            // S' == 0 (p <= q everywhere): the row's greedy id.  Else (r rounded up to S'): the largest j with a positive residual
            int* lastpos = reinterpret_cast<int*>(sh + VERIFY_SH);
            if (t == 0) *lastpos = -1;
            __syncthreads();
            if (last >= 0) atomicMax(lastpos, last);
            __syncthreads();
            token = sh[4] == 0.f ? greedy[row] : *lastpos;
        }
        if (hit >= 0) {
            const int base = hit * SM_CHUNK, len = min(SM_CHUNK, n - base);
            if (DIST && q4) verify_fill_chunk_dist(xf, lg4, q4, base, len, T, mx, sum, t);
            else verify_fill_chunk<true>(xf, lg4, base, len, T, mx, sum, d, t);
            __syncthreads();
            if (t == 0) {
                float cdf = hit ? cend[hit - 1] : 0.f;
                for (int i = 0; i < len; ++i) { cdf = cdf + xf[i]; if (r < cdf) { token = base + i; break; } }
            }
        }
        if (t == 0) out[blockIdx.x] = gl3_verify_result{a, token};
        return;
    }
}

// Draft chain (gl3_forward_decode_chain): the hand-over between step j and step j + 1 of a chain, one launch behind step j's sampler (or
// greedy scan).  id_src = smp_one.res (sampled) or ctx->argmax (greedy): [0] is the step's id.  Thread 0 of workgroup 0 files the id in
// ids[j] and, when a step follows (has_next), makes it that step's input: dyn[0] = id, dyn[1] = next_pos, and on a sampled chain the next
// coin into the SmpRow behind the pair (temperature, topp and mode stay what the host uploaded).  The chain's last step writes no dyn, so dyn
// ends as the last single call's upload would leave it.  q4 != NULL: every workgroup copies its share of the probabilities row (n4 float4s;
// vocab % 16 == 0 at gl3_create) into the target plan's draft table.  The copy is part of this launch, not a hipMemcpyAsync behind it: it
// has to be on the draft plan's stream ahead of the next step's sampler, which overwrites probs, and here it costs no launch of its own.
// Plain vector stores only; nothing in the launch reads what it writes.
__global__ __launch_bounds__(256) void chain_handover_kernel(const int* __restrict__ id_src, int* __restrict__ ids, int j, int* __restrict__ dyn, int has_next, int next_pos,
                                                             const float* __restrict__ coins, const float4* __restrict__ probs4, float4* __restrict__ q4, int n4) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int id = id_src[0];
        ids[j] = id;
        if (has_next) {
            dyn[0] = id; dyn[1] = next_pos;
            if (coins) reinterpret_cast<SmpRow*>(dyn + GL3_DYN_ROW)->coin = coins[j + 1];
        }
    }
    if (q4)
        for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) q4[i] = probs4[i];
}

// Batched draft chain (gl3_forward_decode_batch_chain): the hand-over between step j and step j + 1 of a chain of static-batched steps, one
// launch behind step j's sampler (or greedy scan) whatever the row count.  Grid = (share of the vocabulary, row of the step): the rows of
// step j are the prefix whose k_rows[i] > j (k_rows is non-increasing), and the host launches exactly those.  id_src[id_stride * i] is row
// i's id: the sampler's {token, tie} pairs (stride 2; a greedy row's pair holds the step's greedy id) or, behind a step whose rows are all
// greedy, the step's greedy ids (stride 1).  Thread 0 of a row's first workgroup files the id in ids[j * n + i] and, when the row has a
// further step, makes it that step's input: tokens[i] = id, positions[i] += 1 (the one word this launch reads and writes, by this thread
// alone), and on a chain with sampled rows the next coin into the row's SmpRow (temperature, topp and mode stay what the host staged).  A
// row's last step writes none of the three, so the step's inputs end as the last single call's upload would leave them.  A row with a slot
// (slots[i] >= 0, q4 != NULL): every workgroup of the row copies its share of the probabilities row (n4 float4s; vocab % 16 == 0 at
// gl3_create) into slot slots[i] + j of the target plan's draft table, in this launch for the reason given at chain_handover_kernel.
// Plain vector loads and stores only; no thread reads what another writes.
__global__ __launch_bounds__(256) void batch_chain_handover_kernel(const int* __restrict__ id_src, int id_stride, int* __restrict__ ids, int j, int n,
                                                                   const int* __restrict__ k_rows, const int* __restrict__ slots, int* __restrict__ tokens,
                                                                   int* __restrict__ positions, SmpRow* __restrict__ params, const float* __restrict__ coins,
                                                                   const float4* __restrict__ probs4, float4* __restrict__ q4, int n4) {
    const int i = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int id = id_src[id_stride * i];
        ids[j * n + i] = id;
        if (j + 1 < k_rows[i]) {
            tokens[i] = id; positions[i] = positions[i] + 1;
            if (coins) params[i].coin = coins[(j + 1) * n + i];
        }
    }
    const int slot = q4 ? slots[i] : -1;
    if (slot < 0) return;
    const float4* src = probs4 + (size_t)i * n4;
    float4* dst = q4 + (size_t)(slot + j) * n4;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n4; e += gridDim.x * 256) dst[e] = src[e];
}

// ------------------------------------------------------------------------------------------------ host side
static void sample_drop_graphs(gl3_sample_state* b) {
    for (auto& ge : b->graphs) if (ge) { hipGraphExecDestroy(ge); ge = nullptr; }
}

static void sample_free_buffers(gl3_sample_state* b) {
    sample_drop_graphs(b);
    if (b->probs) hipFree(b->probs);
    if (b->aux) hipFree(b->aux);
    if (b->sort) hipFree(b->sort);
    if (b->res) hipFree(b->res);
    if (b->params) hipFree(b->params);
    if (b->h_params) hipHostFree(b->h_params);
    if (b->h_res) hipHostFree(b->h_res);
    if (b->h_probs) hipHostFree(b->h_probs);
    b->probs = nullptr; b->aux = nullptr; b->sort = nullptr; b->res = nullptr; b->params = nullptr;
    b->h_params = nullptr; b->h_res = nullptr; b->h_probs = nullptr;
    b->rows = 0; b->last_n = 0;
}

static void draft_free(gl3_ctx* ctx) {
    gl3_draft_state* b = &ctx->draft;
    if (b->q) hipFree(b->q);
    if (b->copied) hipEventDestroy(b->copied);
    *b = gl3_draft_state{};
}

static void chain_free(gl3_ctx* ctx) {
    gl3_chain_state* b = &ctx->chain;
    if (b->ids) hipFree(b->ids);
    if (b->coins) hipFree(b->coins);
    if (b->h_ids) hipHostFree(b->h_ids);
    if (b->h_coins) hipHostFree(b->h_coins);
    *b = gl3_chain_state{};
}

static void batch_chain_free(gl3_ctx* ctx) {
    gl3_batch_chain_state* b = &ctx->bchain;
    if (b->ids) hipFree(b->ids);
    if (b->coins) hipFree(b->coins);
    if (b->meta) hipFree(b->meta);
    if (b->h_ids) hipHostFree(b->h_ids);
    if (b->h_coins) hipHostFree(b->h_coins);
    if (b->h_meta) hipHostFree(b->h_meta);
    *b = gl3_batch_chain_state{};
}

void gl3_sample_free(gl3_ctx* ctx) {
    sample_free_buffers(&ctx->smp_one);
    sample_free_buffers(&ctx->smp_rows);
    draft_free(ctx);
    chain_free(ctx);
    batch_chain_free(ctx);
}

static int32_t sample_alloc_all(gl3_ctx* ctx, gl3_sample_state* b, int rows) {
    const size_t vocab = (size_t)ctx->d.vocab;
    const int nchunks = (ctx->d.vocab + SM_CHUNK - 1) / SM_CHUNK, nb = (ctx->d.vocab + RS_TILE - 1) / RS_TILE;
    b->aux_stride = b->blocks + 1 + nchunks;
    b->sort_stride = 4 * vocab + (size_t)256 * nb;
    GL3_HIP(hipMalloc((void**)&b->probs, (size_t)rows * vocab * 4));
    GL3_HIP(hipMalloc((void**)&b->aux, (size_t)rows * b->aux_stride * 4));
    GL3_HIP(hipMalloc((void**)&b->sort, (size_t)rows * b->sort_stride * 4));
    GL3_HIP(hipMalloc((void**)&b->res, (size_t)rows * 3 * sizeof(int)));
    GL3_HIP(hipMalloc((void**)&b->params, (size_t)rows * sizeof(SmpRow)));
    GL3_HIP(hipHostMalloc((void**)&b->h_params, (size_t)rows * sizeof(SmpRow)));
    GL3_HIP(hipHostMalloc((void**)&b->h_res, (size_t)rows * 2 * sizeof(int)));
    GL3_HIP(hipHostMalloc((void**)&b->h_probs, vocab * 4));
    GL3_HIP(hipFuncSetAttribute((const void*)btp_pick_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    GL3_HIP(hipFuncSetAttribute((const void*)bsm_seqsum_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    GL3_HIP(hipFuncSetAttribute((const void*)bsm_seqsum_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    b->rows = rows;
    return GL3_OK;
}

// Every buffer sized for the largest n seen, all or none: a failed allocation (out of memory half way) releases what it got, so the
// next call starts over instead of launching kernels on null pointers.
static int32_t sample_alloc(gl3_ctx* ctx, gl3_sample_state* b, int n) {
    if (b->rows >= n) return GL3_OK;
    if (b->rows) GL3_HIP(hipStreamSynchronize(ctx->stream));      // an earlier step may still read the buffers about to be freed
    sample_free_buffers(b);
    const int32_t r = sample_alloc_all(ctx, b, n);
    if (r != GL3_OK) sample_free_buffers(b);
    return r;
}

static void sample_enqueue(gl3_ctx* ctx, gl3_sample_state* b, const float* logits, RowLayout lay, const int32_t* greedy, const SmpRow* params, int n, bool any_topp) {
    hipStream_t s = ctx->stream;
    const int v = ctx->d.vocab, nb = (v + RS_TILE - 1) / RS_TILE;
    const size_t smem = (size_t)(SM_CHUNK + 32) * 4 + ss_scratch_bytes(SM_CHUNK);
    int* n0 = b->res + 2 * b->rows;
    const dim3 ge(b->blocks, n), gt(nb, n);
    hipLaunchKernelGGL(bsm_scale_max_kernel, ge, dim3(256), 0, s, logits, v, lay, params, greedy, b->probs, b->aux, b->aux_stride, b->res, n0);
    hipLaunchKernelGGL(bsm_exp_kernel, ge, dim3(256), 0, s, b->probs, v, params, b->aux, b->aux_stride, b->blocks);
    hipLaunchKernelGGL(bsm_seqsum_kernel<false>, dim3(n), dim3(256), smem, s, b->probs, v, params, b->aux, b->aux_stride, b->blocks, b->res);
    hipLaunchKernelGGL(bsm_div_kernel, ge, dim3(256), 0, s, b->probs, v, params, b->aux, b->aux_stride, b->blocks);
    hipLaunchKernelGGL(bsm_seqsum_kernel<true>, dim3(n), dim3(256), smem, s, b->probs, v, params, b->aux, b->aux_stride, b->blocks, b->res);
    if (!any_topp) return;
    hipLaunchKernelGGL(btp_keys_kernel, ge, dim3(RS_THREADS), 0, s, b->probs, v, params, b->sort, b->sort_stride, n0);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(btp_hist_kernel, gt, dim3(RS_THREADS), 0, s, params, b->sort, b->sort_stride, v, pass, nb);
        hipLaunchKernelGGL(btp_scan_kernel, dim3(n), dim3(1024), 0, s, params, b->sort, b->sort_stride, v, 256 * nb);
        hipLaunchKernelGGL(btp_scatter_kernel, gt, dim3(RS_THREADS), 0, s, params, b->sort, b->sort_stride, v, pass, nb);
    }
    hipLaunchKernelGGL(btp_pick_kernel, dim3(n), dim3(256), smem, s, params, b->sort, b->sort_stride, v, n0, b->res);
}

// The launches alone, eagerly or as the state's captured graph: what sample_finish and a chained step (gl3_chain_sample) both put on the stream
static int32_t sample_launch(gl3_ctx* ctx, gl3_sample_state* b, const float* logits, RowLayout lay, const int32_t* greedy, const SmpRow* params, int n, bool any_topp) {
    hipStream_t s = ctx->stream;
    static const bool graphs_off = getenv("GL3_NO_GRAPH") && atoi(getenv("GL3_NO_GRAPH"));
    if (b->graph && !graphs_off && !gl3_roctx_on() && !(ctx->d.flags & GL3_FLAG_NO_GRAPH)) {
        if (b->graph_logits != logits || b->graph_greedy != greedy) {      // the step's logits buffer has grown: captured launches point at the old one
            sample_drop_graphs(b);
            b->graph_logits = logits; b->graph_greedy = greedy;
        }
        // A captured launch holds the logits pointer and the layout.  The key covers both: the layout is {vocab / tp, n}, a function of the
        // row count, and the pointer is checked above (one rank: the buffer moves when it grows; tensor parallel: the arena's, it never moves)
        const size_t slot = (size_t)2 * n + (any_topp ? 1 : 0);
        if (b->graphs.size() <= slot) b->graphs.resize(slot + 1, nullptr);
        if (!b->graphs[slot]) {
            hipGraph_t g = nullptr;
            GL3_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            sample_enqueue(ctx, b, logits, lay, greedy, params, n, any_topp);
            GL3_HIP(hipStreamEndCapture(s, &g));
            GL3_HIP(hipGraphInstantiate(&b->graphs[slot], g, nullptr, nullptr, 0));
            hipGraphDestroy(g);
        }
        GL3_HIP(hipGraphLaunch(b->graphs[slot], s));
    } else {
        sample_enqueue(ctx, b, logits, lay, greedy, params, n, any_topp);
    }
    GL3_HIP(hipGetLastError());
    return GL3_OK;
}

// The sampler's launches for rows 0..n) of `logits` (laid out as `lay` says) behind whatever produced them on the plan's stream (params /
// h_params: the rows' settings on the device / the host), 8 * n bytes back, host heap for top-p rows whose flag is set (btp_pick_kernel).
static int32_t sample_finish(gl3_ctx* ctx, gl3_sample_state* b, const float* logits, RowLayout lay, const int32_t* greedy, const SmpRow* params,
                             const SmpRow* h_params, int n, int32_t* tokens_out) {
    hipStream_t s = ctx->stream;
    const int v = ctx->d.vocab;
    static const bool host_topp = env_flag("GL3_TOPP_HOST", false);              // A/B switch: no sort launches, every top-p row through the host heap
    bool any_topp = false;
    for (int i = 0; i < n; ++i) any_topp |= h_params[i].mode == SMP_TOPP && !host_topp;
    int32_t r = sample_launch(ctx, b, logits, lay, greedy, params, n, any_topp);
    if (r != GL3_OK) return r;
    GL3_HIP(hipMemcpyAsync(b->h_res, b->res, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    GL3_HIP(hipStreamSynchronize(s));
    if ((r = gl3_tp_check(ctx)) != GL3_OK) return r;
    b->last_n = n;
    for (int i = 0; i < n; ++i) {
        const SmpRow& R = h_params[i];
        if (R.mode != SMP_TOPP || (!host_topp && !b->h_res[2 * i + 1])) {
            tokens_out[i] = b->h_res[2 * i];
            if (R.mode == SMP_TOPP) ++ctx->topp_device;
            continue;
        }
        // a tie at the sampled rank of this row, or a sum that reaches the heap's own last three: the reference's heap history decides — run it
        GL3_HIP(hipMemcpyAsync(b->h_probs, b->probs + (size_t)i * v, (size_t)v * 4, hipMemcpyDeviceToHost, s));
        GL3_HIP(hipStreamSynchronize(s));
        tokens_out[i] = topp_sample(b->h_probs, v, R.topp, R.coin, ctx->topp_indices);
        ++ctx->topp_host;
    }
    return GL3_OK;
}

// ---- single-row entry: logits (device, f32[vocab], complete on this rank) -> sampled id.  The row's settings were uploaded behind the
// (token, position) pair by the step's own copy (set_dyn, gl3_api.hip); never greedy (temperature > 0), so no greedy ids are passed.
int32_t gl3_sample_run(gl3_ctx* ctx, const float* logits_dev, int32_t* token_out) {
    const int32_t r = sample_alloc(ctx, &ctx->smp_one, 1);
    if (r != GL3_OK) return r;
    return sample_finish(ctx, &ctx->smp_one, logits_dev, RowLayout{ctx->d.vocab, 1}, nullptr, reinterpret_cast<const SmpRow*>(ctx->dyn + GL3_DYN_ROW), reinterpret_cast<const SmpRow*>(ctx->h_dyn + GL3_DYN_ROW), 1, token_out);
}

int32_t gl3_sample_probs(gl3_ctx* ctx, float* out) {       // parity tap: the probabilities of the last single-row sampled step
    if (!ctx->smp_one.last_n) GL3_FAIL(GL3_E_STATE, "no sampled step yet");
    GL3_HIP(hipMemcpy(out, ctx->smp_one.probs, (size_t)ctx->d.vocab * 4, hipMemcpyDeviceToHost));
    return GL3_OK;
}

// ---- batched entries: prepare = check + stage the per-row settings (before the step is enqueued), finish = the launches behind it
int32_t gl3_sample_batch_prepare(gl3_ctx* ctx, int32_t n, const float* temperature, const float* topp, const float* coins, bool* all_greedy) {
    gl3_sample_state* b = &ctx->smp_rows;
    bool any = false;
    for (int i = 0; i < n; ++i) {
        if (!(temperature[i] >= 0.f)) GL3_FAIL(GL3_E_ARG, "temperature must be >= 0");
        if (temperature[i] == 0.f) continue;                          // Sampler.java:79-81: greedy argmax; the row's coin is not looked at
        if (!(coins[i] >= 0.f && coins[i] < 1.f)) GL3_FAIL(GL3_E_ARG, "coin must be rng.nextFloat(1f): in [0, 1)");
        any = true;
    }
    *all_greedy = !any;
    b->last_n = 0;
    if (!any) return GL3_OK;                                          // the step's own greedy ids answer every row: nothing to stage
    GL3_HIP(hipSetDevice(ctx->d.device));
    const int32_t r = sample_alloc(ctx, b, n);
    if (r != GL3_OK) return r;
    for (int i = 0; i < n; ++i) b->h_params[i] = gl3_smp_row(temperature[i], topp[i], coins[i]);
    GL3_HIP(hipMemcpyAsync(b->params, b->h_params, (size_t)n * sizeof(SmpRow), hipMemcpyHostToDevice, ctx->stream));
    return GL3_OK;
}

int32_t gl3_sample_batch_finish(gl3_ctx* ctx, const float* logits_dev, const int32_t* greedy_dev, int32_t n, int32_t* tokens_out) {
    gl3_sample_state* b = &ctx->smp_rows;
    // a batched step's logits: rank-chunked [tp][n][vocab / tp] (one rank: plain rows), complete on every rank, which samples them redundantly
    return sample_finish(ctx, b, logits_dev, RowLayout{ctx->vocab_l, n}, greedy_dev, b->params, b->h_params, n, tokens_out);
}

int32_t gl3_sample_probs_row(gl3_ctx* ctx, int32_t row, float* out) {      // parity tap: what row `row` of the last batched sampled step was drawn from
    const gl3_sample_state* b = &ctx->smp_rows;
    if (!b->last_n) GL3_FAIL(GL3_E_STATE, "no batched sampled step yet");
    if (row < 0 || row >= b->last_n) GL3_FAIL(GL3_E_ARG, "row outside the last batched sampled step");
    if (b->h_params[row].mode == SMP_GREEDY) GL3_FAIL(GL3_E_STATE, "the row was greedy: it has no probabilities");
    GL3_HIP(hipMemcpy(out, b->probs + (size_t)row * ctx->d.vocab, (size_t)ctx->d.vocab * 4, hipMemcpyDeviceToHost));
    return GL3_OK;
}

// ---- token scores: prepare = every check + stage the rows' settings (before the step is enqueued), finish = the one launch behind the
// step on the plan's stream and 16 * n bytes back in one copy
void gl3_score_free(gl3_ctx* ctx) {
    gl3_score_state* b = &ctx->score;
    if (b->params) hipFree(b->params);
    if (b->out) hipFree(b->out);
    if (b->h_params) hipHostFree(b->h_params);
    if (b->h_out) hipHostFree(b->h_out);
    if (b->ev0) hipEventDestroy(b->ev0);
    if (b->ev1) hipEventDestroy(b->ev1);
    *b = gl3_score_state{};
}

int32_t gl3_score_prepare(gl3_ctx* ctx, int32_t n, const int32_t* targets, const float* temperature) {
    gl3_score_state* b = &ctx->score;
    if (!targets) GL3_FAIL(GL3_E_ARG, "null targets");
    for (int i = 0; i < n; ++i) {
        if (targets[i] < 0 || targets[i] >= ctx->d.vocab) GL3_FAIL(GL3_E_ARG, "target id out of range");
        if (temperature && !(temperature[i] > 0.f)) GL3_FAIL(GL3_E_ARG, "temperature must be > 0");
    }
    GL3_HIP(hipSetDevice(ctx->d.device));
    if (b->rows < n) {      // all or none, as sample_alloc
        if (b->rows) GL3_HIP(hipStreamSynchronize(ctx->stream));
        gl3_score_free(ctx);
        hipError_t e = hipMalloc((void**)&b->params, (size_t)n * sizeof(ScoreRow));
        if (e == hipSuccess) e = hipMalloc((void**)&b->out, (size_t)n * sizeof(gl3_token_score));
        if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_params, (size_t)n * sizeof(ScoreRow));
        if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_out, (size_t)n * sizeof(gl3_token_score));
        if (e != hipSuccess) { gl3_score_free(ctx); GL3_HIP(e); }
        b->rows = n;
    }
    for (int i = 0; i < n; ++i) b->h_params[i] = ScoreRow{targets[i], temperature ? temperature[i] : 1.f};
    GL3_HIP(hipMemcpyAsync(b->params, b->h_params, (size_t)n * sizeof(ScoreRow), hipMemcpyHostToDevice, ctx->stream));
    return GL3_OK;
}

int32_t gl3_score_finish(gl3_ctx* ctx, const float* logits_dev, int32_t n, gl3_token_score* scores_out) {
    gl3_score_state* b = &ctx->score;
    hipStream_t s = ctx->stream;
    const size_t smem = (size_t)(SM_CHUNK + 32) * 4 + ss_scratch_bytes(SM_CHUNK) + 32;
    static const bool timed = env_flag("GL3_SCORE_TIMING", false);      // measurement switch: HIP events around the launch, its device time on stderr
    if (timed && !b->ev0) { GL3_HIP(hipEventCreate(&b->ev0)); GL3_HIP(hipEventCreate(&b->ev1)); }
    if (timed) GL3_HIP(hipEventRecord(b->ev0, s));
    hipLaunchKernelGGL(score_rows_kernel, dim3(n), dim3(256), smem, s, logits_dev, ctx->d.vocab, RowLayout{ctx->vocab_l, n}, b->params, b->out);
    if (timed) GL3_HIP(hipEventRecord(b->ev1, s));
    GL3_HIP(hipGetLastError());
    GL3_HIP(hipMemcpyAsync(b->h_out, b->out, (size_t)n * sizeof(gl3_token_score), hipMemcpyDeviceToHost, s));
    GL3_HIP(hipStreamSynchronize(s));
    const int32_t r = gl3_tp_check(ctx);
    if (r != GL3_OK) return r;
    if (timed) {
        float ms = 0.f;
        GL3_HIP(hipEventElapsedTime(&ms, b->ev0, b->ev1));
        fprintf(stderr, "gl3 score_rows_kernel rows %d: %.1f us\n", n, ms * 1e3);
    }
    memcpy(scores_out, b->h_out, (size_t)n * sizeof(gl3_token_score));
    return GL3_OK;
}

// ---- draft verification: prepare = every check + stage the runs and rows (before the step is enqueued), enqueue = the one launch behind
// the step on the plan's stream and the copy of 8 * n_runs bytes, collect = wait for both
void gl3_verify_free(gl3_ctx* ctx) {
    gl3_verify_state* b = &ctx->verify;
    if (b->params) hipFree(b->params);
    if (b->out) hipFree(b->out);
    if (b->h_params) hipHostFree(b->h_params);
    if (b->h_out) hipHostFree(b->h_out);
    *b = gl3_verify_state{};
}

// ---- draft distributions of a target plan: q[max_batch][vocab], the table and its event on the first put, all or none
static int32_t draft_slot(gl3_ctx* ctx, int32_t slot, float** row) {
    gl3_draft_state* b = &ctx->draft;
    GL3_HIP(hipSetDevice(ctx->d.device));
    if (!b->q) {
        hipError_t e = hipMalloc((void**)&b->q, (size_t)ctx->d.max_batch * ctx->d.vocab * 4);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&b->copied, hipEventDisableTiming);
        if (e != hipSuccess) { draft_free(ctx); GL3_HIP(e); }
        b->written.assign((size_t)ctx->d.max_batch, 0);
    }
    *row = b->q + (size_t)slot * ctx->d.vocab;
    return GL3_OK;
}

// One device-to-device copy on the TARGET's stream, behind whatever the target enqueued last.  The draft plan's forward has returned, so
// its stream is idle and the row is complete; the draft's stream then waits for the copy, so its next sampled step cannot overwrite the
// row under it.  Nothing waits on the host.
int32_t gl3_draft_put(gl3_ctx* ctx, int32_t slot, gl3_ctx* draft) {
    float* row = nullptr;
    const int32_t r = draft_slot(ctx, slot, &row);
    if (r != GL3_OK) return r;
    GL3_HIP(hipMemcpyAsync(row, draft->smp_one.probs, (size_t)ctx->d.vocab * 4, hipMemcpyDeviceToDevice, ctx->stream));
    GL3_HIP(hipEventRecord(ctx->draft.copied, ctx->stream));
    GL3_HIP(hipStreamWaitEvent(draft->stream, ctx->draft.copied, 0));
    ctx->draft.written[slot] = 1;
    return GL3_OK;
}

int32_t gl3_draft_put_host(gl3_ctx* ctx, int32_t slot, const float* q) {
    float* row = nullptr;
    const int32_t r = draft_slot(ctx, slot, &row);
    if (r != GL3_OK) return r;
    GL3_HIP(hipMemcpyAsync(row, q, (size_t)ctx->d.vocab * 4, hipMemcpyHostToDevice, ctx->stream));
    GL3_HIP(hipStreamSynchronize(ctx->stream));      // q is the caller's (pageable) memory: done with it on return
    ctx->draft.written[slot] = 1;
    return GL3_OK;
}

int32_t gl3_draft_get(gl3_ctx* ctx, int32_t slot, float* out) {
    const gl3_draft_state* b = &ctx->draft;
    if (!b->q || !b->written[slot]) GL3_FAIL(GL3_E_STATE, "the draft-distribution slot was never written");
    GL3_HIP(hipSetDevice(ctx->d.device));
    GL3_HIP(hipMemcpyAsync(out, b->q + (size_t)slot * ctx->d.vocab, (size_t)ctx->d.vocab * 4, hipMemcpyDeviceToHost, ctx->stream));
    GL3_HIP(hipStreamSynchronize(ctx->stream));
    return GL3_OK;
}

// ---- draft chain (gl3_forward_decode_chain; every argument check is gl3_api.hip's and has passed): k single-token steps on the plan's
// stream, step j + 1 fed by chain_handover_kernel behind step j, one wait at the end
int32_t gl3_chain_prepare(gl3_ctx* ctx, int32_t k, const float* coins, gl3_ctx* target, int32_t slot0, float** q_row0) {
    gl3_chain_state* b = &ctx->chain;
    GL3_HIP(hipSetDevice(ctx->d.device));
    if (!b->ids) {      // once, for the longest chain; all or none, as gl3_verify_prepare
        hipError_t e = hipMalloc((void**)&b->ids, GL3_CHAIN_MAX * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void**)&b->coins, GL3_CHAIN_MAX * sizeof(float));
        if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_ids, GL3_CHAIN_MAX * sizeof(int));
        if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_coins, GL3_CHAIN_MAX * sizeof(float));
        if (e != hipSuccess) { chain_free(ctx); GL3_HIP(e); }
    }
    if (coins) {
        const int32_t r = sample_alloc(ctx, &ctx->smp_one, 1);
        if (r != GL3_OK) return r;
    }
    *q_row0 = nullptr;
    if (target) {
        const int32_t r = draft_slot(target, slot0, q_row0);
        if (r != GL3_OK) { ctx->err = target->err; return r; }
        // the rows are written on THIS plan's stream: behind whatever the target's stream still holds (a gl3_draft_probs_put of another
        // draft into the same table).  The call returns after its own wait, so the target needs no event for what follows.
        GL3_HIP(hipEventRecord(target->draft.copied, target->stream));
        GL3_HIP(hipStreamWaitEvent(ctx->stream, target->draft.copied, 0));
    }
    if (coins) {
        memcpy(b->h_coins, coins, (size_t)k * sizeof(float));
        GL3_HIP(hipMemcpyAsync(b->coins, b->h_coins, (size_t)k * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    return GL3_OK;
}

// the single-row sampler behind a chained step: gl3_sample_run's launches (never top-p), without its copy and wait
int32_t gl3_chain_sample(gl3_ctx* ctx) {
    return sample_launch(ctx, &ctx->smp_one, ctx->logits, RowLayout{ctx->d.vocab, 1}, nullptr, reinterpret_cast<const SmpRow*>(ctx->dyn + GL3_DYN_ROW), 1, false);
}

int32_t gl3_chain_handover(gl3_ctx* ctx, int32_t j, int32_t k, int32_t next_pos, bool sampled, float* q_row) {
    const gl3_chain_state* b = &ctx->chain;
    const int n4 = ctx->d.vocab / 4;
    const int wgs = q_row ? std::min((n4 + 255) / 256, 256) : 1;
    hipLaunchKernelGGL(chain_handover_kernel, dim3(wgs), dim3(256), 0, ctx->stream, sampled ? ctx->smp_one.res : ctx->argmax, b->ids, j, ctx->dyn, j + 1 < k ? 1 : 0, next_pos,
                       sampled ? b->coins : (const float*)nullptr, reinterpret_cast<const float4*>(ctx->smp_one.probs), reinterpret_cast<float4*>(q_row), n4);
    GL3_HIP(hipGetLastError());
    return GL3_OK;
}

int32_t gl3_chain_collect(gl3_ctx* ctx, int32_t k, bool sampled, gl3_ctx* target, int32_t slot0, int32_t* tokens_out) {
    gl3_chain_state* b = &ctx->chain;
    GL3_HIP(hipMemcpyAsync(b->h_ids, b->ids, (size_t)k * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GL3_HIP(hipStreamSynchronize(ctx->stream));
    const int32_t r = gl3_tp_check(ctx);
    if (r != GL3_OK) return r;
    if (sampled) ctx->smp_one.last_n = 1;
    for (int j = 0; target && j < k; ++j) target->draft.written[slot0 + j] = 1;
    memcpy(tokens_out, b->h_ids, (size_t)k * sizeof(int));
    return GL3_OK;
}

// ---- one slot of a target's table from a row of the draft plan's batched sampler: gl3_draft_put with smp_rows.probs row `row` as the source
int32_t gl3_draft_put_row(gl3_ctx* ctx, int32_t slot, gl3_ctx* draft, int32_t row) {
    float* dst = nullptr;
    const int32_t r = draft_slot(ctx, slot, &dst);
    if (r != GL3_OK) return r;
    GL3_HIP(hipMemcpyAsync(dst, draft->smp_rows.probs + (size_t)row * ctx->d.vocab, (size_t)ctx->d.vocab * 4, hipMemcpyDeviceToDevice, ctx->stream));
    GL3_HIP(hipEventRecord(ctx->draft.copied, ctx->stream));
    GL3_HIP(hipStreamWaitEvent(draft->stream, ctx->draft.copied, 0));
    ctx->draft.written[slot] = 1;
    return GL3_OK;
}

// ---- batched draft chain (gl3_forward_decode_batch_chain; every argument check is gl3_api.hip's and has passed): k static-batched steps on
// the plan's stream, step j + 1 fed by batch_chain_handover_kernel behind step j, one wait at the end.  Row i takes k_i = k_rows[i] (NULL: k)
// steps; the lists are [step][row] with stride n.
int32_t gl3_batch_chain_prepare(gl3_ctx* ctx, int32_t n, int32_t k, const int32_t* k_rows, const float* temperature, const float* coins, gl3_ctx* target,
                                const int32_t* slots) {
    gl3_batch_chain_state* b = &ctx->bchain;
    ctx->smp_rows.last_n = 0;      // as gl3_sample_batch_prepare: a chain that fails midway leaves no row of a half-run step to hand out
    GL3_HIP(hipSetDevice(ctx->d.device));
    if (!b->ids) {      // once, for the longest chain of the widest step; all or none, as gl3_chain_prepare
        const size_t cap = (size_t)GL3_CHAIN_MAX * ctx->d.max_batch, mcap = (size_t)2 * ctx->d.max_batch;
        hipError_t e = hipMalloc((void**)&b->ids, cap * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void**)&b->coins, cap * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&b->meta, mcap * sizeof(int));
        if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_ids, cap * sizeof(int));
        if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_coins, cap * sizeof(float));
        if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_meta, mcap * sizeof(int));
        if (e != hipSuccess) { batch_chain_free(ctx); GL3_HIP(e); }
    }
    bool any = false;
    for (int i = 0; i < n; ++i) any |= temperature[i] > 0.f;
    b->sampled = any;
    gl3_sample_state* sm = &ctx->smp_rows;
    if (any) {      // step 0's gl3_sample_batch_prepare: the rows' settings with the step-0 coins
        const int32_t r = sample_alloc(ctx, sm, n);
        if (r != GL3_OK) return r;
        for (int i = 0; i < n; ++i) sm->h_params[i] = gl3_smp_row(temperature[i], 0.f, temperature[i] > 0.f ? coins[i] : 0.f);
        GL3_HIP(hipMemcpyAsync(sm->params, sm->h_params, (size_t)n * sizeof(SmpRow), hipMemcpyHostToDevice, ctx->stream));
    }
    if (target) {
        float* q0 = nullptr;
        const int32_t r = draft_slot(target, 0, &q0);
        if (r != GL3_OK) { ctx->err = target->err; return r; }
        // as gl3_chain_prepare: the rows are written on THIS plan's stream, behind whatever the target's stream still holds
        GL3_HIP(hipEventRecord(target->draft.copied, target->stream));
        GL3_HIP(hipStreamWaitEvent(ctx->stream, target->draft.copied, 0));
    }
    for (int i = 0; i < n; ++i) {
        const int ki = k_rows ? k_rows[i] : k;
        b->h_meta[i] = ki;
        b->h_meta[n + i] = target ? slots[i] : -1;
        for (int j = 0; j < k; ++j) b->h_coins[(size_t)j * n + i] = temperature[i] > 0.f && j < ki ? coins[(size_t)j * n + i] : 0.f;
    }
    GL3_HIP(hipMemcpyAsync(b->meta, b->h_meta, (size_t)2 * n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (any) GL3_HIP(hipMemcpyAsync(b->coins, b->h_coins, (size_t)k * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    return GL3_OK;
}

// the batched sampler behind a chained step of nj rows: gl3_sample_batch_finish's launches (never top-p), without its copy and wait
int32_t gl3_batch_chain_sample(gl3_ctx* ctx, const float* logits_dev, const int32_t* greedy_dev, int32_t nj) {
    gl3_sample_state* sm = &ctx->smp_rows;
    return sample_launch(ctx, sm, logits_dev, RowLayout{ctx->vocab_l, nj}, greedy_dev, sm->params, nj, false);
}

int32_t gl3_batch_chain_handover(gl3_ctx* ctx, int32_t j, int32_t n, int32_t nj, bool sampled_step, const int32_t* greedy_dev, int32_t* tokens_dev,
                                 int32_t* positions_dev, gl3_ctx* target) {
    const gl3_batch_chain_state* b = &ctx->bchain;
    const gl3_sample_state* sm = &ctx->smp_rows;
    const int n4 = ctx->d.vocab / 4;
    bool copies = false;                                  // a row of this step has a slot (only a sampled row can: the step then ran the sampler)
    for (int i = 0; i < nj; ++i) copies |= b->h_meta[n + i] >= 0;
    const int wgs = copies ? std::min((n4 + 255) / 256, 64) : 1;
    hipLaunchKernelGGL(batch_chain_handover_kernel, dim3(wgs, nj), dim3(256), 0, ctx->stream, sampled_step ? sm->res : greedy_dev, sampled_step ? 2 : 1, b->ids, j, n,
                       b->meta, b->meta + n, tokens_dev, positions_dev, sm->params, b->sampled ? b->coins : (const float*)nullptr,
                       reinterpret_cast<const float4*>(sm->probs), copies ? reinterpret_cast<float4*>(target->draft.q) : (float4*)nullptr, n4);
    GL3_HIP(hipGetLastError());
    return GL3_OK;
}

int32_t gl3_batch_chain_collect(gl3_ctx* ctx, int32_t n, int32_t k, const int32_t* k_rows, const float* temperature, gl3_ctx* target, const int32_t* slots,
                                int32_t* tokens_out) {
    gl3_batch_chain_state* b = &ctx->bchain;
    gl3_sample_state* sm = &ctx->smp_rows;
    GL3_HIP(hipMemcpyAsync(b->h_ids, b->ids, (size_t)k * n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GL3_HIP(hipStreamSynchronize(ctx->stream));
    const int32_t r = gl3_tp_check(ctx);
    if (r != GL3_OK) return r;
    for (int j = 0; j < k; ++j) {
        // the host's copy of the sampler state as the single call of step j leaves it: the rows' settings with the step's coins and the
        // step's row count; a step whose rows are all greedy has no sampled rows (gl3_sample_batch_prepare)
        int nj = 0;
        bool any = false;
        for (int i = 0; i < n && (k_rows ? k_rows[i] : k) > j; ++i) { ++nj; any |= temperature[i] > 0.f; }
        for (int i = 0; any && i < nj; ++i) sm->h_params[i] = gl3_smp_row(temperature[i], 0.f, b->h_coins[(size_t)j * n + i]);
        sm->last_n = any ? nj : 0;
        for (int i = 0; i < n; ++i) {
            tokens_out[(size_t)j * n + i] = i < nj ? b->h_ids[(size_t)j * n + i] : -1;
            if (target && i < nj && slots[i] >= 0) target->draft.written[slots[i] + j] = 1;
        }
    }
    return GL3_OK;
}

int32_t gl3_verify_prepare(gl3_ctx* ctx, int32_t n, const int32_t* tokens, const float* coins, int32_t n_runs, const int32_t* run_row0,
                           const int32_t* run_rows, const float* temperature, bool dist, const int32_t* q_slots) {
    gl3_verify_state* b = &ctx->verify;
    if (dist && !q_slots) GL3_FAIL(GL3_E_ARG, "null q_slots");
    for (int k = 0; k < n_runs; ++k) {
        const float T = temperature ? temperature[k] : 0.f;
        if (!(T >= 0.f)) GL3_FAIL(GL3_E_ARG, "temperature must be >= 0");
        if (T == 0.f) continue;                                       // greedy: the run's coins are not looked at
        if (!coins) GL3_FAIL(GL3_E_ARG, "null coins with a run at a temperature > 0");
        for (int i = 2 * run_row0[k]; i < 2 * (run_row0[k] + run_rows[k]); ++i)
            if (!(coins[i] >= 0.f && coins[i] < 1.f)) GL3_FAIL(GL3_E_ARG, "coin must be rng.nextFloat(1f): in [0, 1)");
    }
    // q_slots of the rows that look at them: the rows of a sampled run that have a draft (all but the run's last).  Range first, for every
    // such row, then whether the slot was ever put
    for (int pass = 0; dist && pass < 2; ++pass)
        for (int k = 0; k < n_runs; ++k) {
            if (!temperature || temperature[k] == 0.f) continue;
            for (int i = run_row0[k]; i + 1 < run_row0[k] + run_rows[k]; ++i) {
                const int32_t s = q_slots[i];
                if (pass == 0 && (s < -1 || s >= ctx->d.max_batch)) GL3_FAIL(GL3_E_ARG, "q_slots entry outside [-1, max_batch)");
                if (pass == 1 && s >= 0 && !(ctx->draft.q && ctx->draft.written[s])) GL3_FAIL(GL3_E_STATE, "q_slots names a draft-distribution slot that was never written");
            }
        }
    GL3_HIP(hipSetDevice(ctx->d.device));
    if (!b->cap) {      // once, for the largest step the plan takes (a run has at least one row); all or none, as sample_alloc
        const size_t cap = (size_t)ctx->d.max_batch, bytes = cap * (sizeof(VerifyRun) + sizeof(VerifyRow));
        hipError_t e = hipMalloc((void**)&b->params, bytes);
        if (e == hipSuccess) e = hipMalloc((void**)&b->out, cap * sizeof(gl3_verify_result));
        if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_params, bytes);
        if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_out, cap * sizeof(gl3_verify_result));
        if (e != hipSuccess) { gl3_verify_free(ctx); GL3_HIP(e); }
        b->cap = (int)cap;
    }
    VerifyRun* hr = reinterpret_cast<VerifyRun*>(b->h_params);      // the n rows lie right behind the n_runs runs: one copy of what the step uses
    VerifyRow* hw = reinterpret_cast<VerifyRow*>(b->h_params + (size_t)n_runs * sizeof(VerifyRun));
    for (int k = 0; k < n_runs; ++k) hr[k] = VerifyRun{run_row0[k], run_rows[k], temperature ? temperature[k] : 0.f, 0};
    for (int i = 0; i < n; ++i) hw[i] = VerifyRow{tokens[i], coins ? coins[2 * i] : 0.f, coins ? coins[2 * i + 1] : 0.f, dist ? q_slots[i] : -1};
    GL3_HIP(hipMemcpyAsync(b->params, b->h_params, (size_t)n_runs * sizeof(VerifyRun) + (size_t)n * sizeof(VerifyRow), hipMemcpyHostToDevice, ctx->stream));
    return GL3_OK;
}

int32_t gl3_verify_enqueue(gl3_ctx* ctx, const float* logits_dev, const int32_t* greedy_dev, int32_t n_runs, bool dist) {
    gl3_verify_state* b = &ctx->verify;
    hipStream_t s = ctx->stream;
    const int v = ctx->d.vocab, nchunks = (v + SM_CHUNK - 1) / SM_CHUNK;
    const VerifyRun* runs = reinterpret_cast<const VerifyRun*>(b->params);
    const VerifyRow* rows = reinterpret_cast<const VerifyRow*>(b->params + (size_t)n_runs * sizeof(VerifyRun));
    // the draft table may not exist (every q_slots entry -1): no row then looks at it
    if (dist) hipLaunchKernelGGL(verify_runs_kernel<true>, dim3(n_runs), dim3(256), verify_smem(nchunks, true), s, logits_dev, v, runs, rows, greedy_dev, b->out, ctx->draft.q);
    else hipLaunchKernelGGL(verify_runs_kernel<false>, dim3(n_runs), dim3(256), verify_smem(nchunks, false), s, logits_dev, v, runs, rows, greedy_dev, b->out, (const float*)nullptr);
    GL3_HIP(hipGetLastError());
    GL3_HIP(hipMemcpyAsync(b->h_out, b->out, (size_t)n_runs * sizeof(gl3_verify_result), hipMemcpyDeviceToHost, s));
    return GL3_OK;
}

int32_t gl3_verify_collect(gl3_ctx* ctx, int32_t n_runs, gl3_verify_result* results_out) {
    GL3_HIP(hipStreamSynchronize(ctx->stream));
    const int32_t r = gl3_tp_check(ctx);
    if (r != GL3_OK) return r;
    memcpy(results_out, ctx->verify.h_out, (size_t)n_runs * sizeof(gl3_verify_result));
    return GL3_OK;
}
