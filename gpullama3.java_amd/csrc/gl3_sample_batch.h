// gl3_sample_batch.h — the samplers of gl3_sample.hip for every row of a static-batched decode step (included by gl3_sample.hip).
//
// The arithmetic of a row is that of the single-row pipeline, step for step (see the header of gl3_sample.hip); what changes is the
// shape of the launches: rows are a grid dimension, so a step costs the same 19 launches at every batch size —
//     bsm_scale_max, bsm_exp, bsm_seqsum<false>, bsm_div, bsm_seqsum<true> (categorical pick),
//     btp_keys, 4 x (btp_hist, btp_scan, btp_scatter), btp_pick                      (left out when no row of the step uses top-p)
// and every per-row setting (temperature, topp, coin, mode) is read from a small device array staged with the step's tokens, so no
// kernel takes a per-step scalar and the launches replay as one hipGraph per batch size.  A row whose mode does not need a stage
// returns at once in that stage: greedy rows take the id of the step's own greedy scan (pf_argmax_*), categorical rows skip the sort.
// The sequential sums keep one workgroup per row (n rows run side by side on n CUs); the radix sort is segmented by row (histogram
// [row][digit][tile], one scan workgroup per row, stable scatter inside the row).  {token, tie} of every row come back in one copy of
// 8 * n bytes; only rows whose tie flag is set have their probabilities copied out and run through the host heap (topp_sample).
// The logits are read, never written.
#pragma once

enum { SMP_GREEDY = 0, SMP_CATEGORICAL = 1, SMP_TOPP = 2 };
struct SmpRow { float temperature, topp, coin; int mode; };

constexpr int BSM_BLOCKS = 64;                 // workgroups per row of the element-wise stages

struct gl3_bsample_state {
    int rows = 0;                              // capacity of every buffer below
    float* probs = nullptr;                    // [rows][vocab]
    float* aux = nullptr;                      // [rows][aux_stride]: BSM_BLOCKS block maxima, the total, nchunks chunk ends
    int aux_stride = 0;
    uint32_t* sort = nullptr;                  // [rows][4 vocab + 256 nb]: (keys, indices) x 2, radix histogram
    size_t sort_stride = 0;
    int* res = nullptr;                        // [rows][2] {token, tie}, then [rows] n0 (top-p candidates)
    SmpRow* params = nullptr;                  // [rows]
    SmpRow* h_params = nullptr;                // pinned
    int* h_res = nullptr;                      // pinned [rows][2]
    float* h_probs = nullptr;                  // pinned [vocab]: one tied row at a time
    std::vector<hipGraphExec_t> graphs;        // [2 n + (any top-p row)]
    const float* graph_logits = nullptr;       // the pointers the captured launches hold
    const int32_t* graph_greedy = nullptr;
    int last_n = 0;                            // rows of the last sampled step (their modes: h_params)
};

__global__ __launch_bounds__(256) void bsm_scale_max_kernel(const float* __restrict__ logits, int n, const SmpRow* __restrict__ rows, const int32_t* __restrict__ greedy,
                                                            float* __restrict__ probs, float* __restrict__ aux, int aux_stride, int* __restrict__ res, int* __restrict__ n0) {
    __shared__ float red[4];
    const int row = blockIdx.y;
    const SmpRow R = rows[row];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        n0[row] = 0;
        if (R.mode == SMP_GREEDY) { res[2 * row] = greedy[row]; res[2 * row + 1] = 0; }
    }
    if (R.mode == SMP_GREEDY) return;
    const float* lg = logits + (size_t)row * n;
    float* p = probs + (size_t)row * n;
    float mx = -INFINITY;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float v = lg[i] / R.temperature;                         // divideInPlace(temperature)
        p[i] = v;
        mx = fmaxf(mx, v);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) aux[(size_t)row * aux_stride + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void bsm_exp_kernel(float* __restrict__ probs, int n, const SmpRow* __restrict__ rows, const float* __restrict__ aux, int aux_stride) {
    __shared__ float red[4];
    const int row = blockIdx.y;
    if (rows[row].mode == SMP_GREEDY) return;
    float* p = probs + (size_t)row * n;
    const float* blockmax = aux + (size_t)row * aux_stride;
    float mx = threadIdx.x < BSM_BLOCKS ? blockmax[threadIdx.x] : -INFINITY;
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) p[i] = (float)exp((double)(p[i] - mx));   // (float) Math.exp(f - maxVal)
}

// smp_seqsum_kernel, one workgroup per row.  PICK = false: every non-greedy row, total and chunk ends of the numerators;
// PICK = true: categorical rows only, res[row] = {first index whose cdf exceeds the row's coin, 0}.
template <bool PICK>
__global__ __launch_bounds__(256) void bsm_seqsum_kernel(const float* __restrict__ probs, int n, const SmpRow* __restrict__ rows, float* __restrict__ aux, int aux_stride,
                                                         int* __restrict__ res) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* xf = reinterpret_cast<float*>(smem);                      // [SM_CHUNK + 32]
    uint8_t* scratch = smem + (size_t)(SM_CHUNK + 32) * 4;
    __shared__ float run_s;
    __shared__ int hit_s;
    const int row = blockIdx.x;
    const SmpRow R = rows[row];
    if (PICK ? R.mode != SMP_CATEGORICAL : R.mode == SMP_GREEDY) return;
    const float* p = probs + (size_t)row * n;
    float* total = aux + (size_t)row * aux_stride + BSM_BLOCKS;
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

__global__ __launch_bounds__(256) void bsm_div_kernel(float* __restrict__ probs, int n, const SmpRow* __restrict__ rows, const float* __restrict__ aux, int aux_stride) {
    const int row = blockIdx.y;
    if (rows[row].mode == SMP_GREEDY) return;
    float* p = probs + (size_t)row * n;
    const float s = aux[(size_t)row * aux_stride + BSM_BLOCKS];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) p[i] = p[i] / s;     // divideInPlace(sum)
}

// ---- top-p rows: the radix sort of gl3_sample.hip, segmented by row.  A row's segment of `sort`: ka[n] ia[n] kb[n] ib[n] hist[256 nb].
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

// topp_pick_kernel, one workgroup per row: res[row] = {index at the chosen rank, tie flag}
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
        out[1] = tie ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ host side
static void bsample_drop_graphs(gl3_bsample_state* b) {
    for (auto& ge : b->graphs) if (ge) { hipGraphExecDestroy(ge); ge = nullptr; }
}

static void bsample_free_buffers(gl3_bsample_state* b) {
    bsample_drop_graphs(b);
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

void gl3_sample_batch_free(gl3_ctx* ctx) {
    if (!ctx->bs) return;
    bsample_free_buffers(ctx->bs);
    delete ctx->bs;
    ctx->bs = nullptr;
}

static int32_t bsample_alloc_all(gl3_ctx* ctx, int rows) {
    gl3_bsample_state* b = ctx->bs;
    const size_t vocab = (size_t)ctx->d.vocab;
    const int nchunks = (ctx->d.vocab + SM_CHUNK - 1) / SM_CHUNK, nb = (ctx->d.vocab + RS_TILE - 1) / RS_TILE;
    b->aux_stride = BSM_BLOCKS + 1 + nchunks;
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

// Every buffer sized for the largest n seen, all or none (as gl3_sample_alloc): a failed allocation releases what it got.
static int32_t bsample_alloc(gl3_ctx* ctx, int n) {
    if (!ctx->bs) ctx->bs = new gl3_bsample_state();
    if (ctx->bs->rows >= n) return GL3_OK;
    GL3_HIP(hipStreamSynchronize(ctx->stream));
    bsample_free_buffers(ctx->bs);
    const int32_t r = bsample_alloc_all(ctx, n);
    if (r != GL3_OK) bsample_free_buffers(ctx->bs);
    return r;
}

int32_t gl3_sample_batch_prepare(gl3_ctx* ctx, int32_t n, const float* temperature, const float* topp, const float* coins, bool* all_greedy) {
    bool any = false;
    for (int i = 0; i < n; ++i) {
        if (!(temperature[i] >= 0.f)) GL3_FAIL(GL3_E_ARG, "temperature must be >= 0");
        if (temperature[i] == 0.f) continue;                          // Sampler.java:79-81: greedy argmax; the row's coin is not looked at
        if (!(coins[i] >= 0.f && coins[i] < 1.f)) GL3_FAIL(GL3_E_ARG, "coin must be rng.nextFloat(1f): in [0, 1)");
        any = true;
    }
    *all_greedy = !any;
    if (ctx->bs) ctx->bs->last_n = 0;
    if (!any) return GL3_OK;                                          // the step's own greedy ids answer every row: nothing to stage
    GL3_HIP(hipSetDevice(ctx->d.device));
    const int32_t r = bsample_alloc(ctx, n);
    if (r != GL3_OK) return r;
    gl3_bsample_state* b = ctx->bs;
    for (int i = 0; i < n; ++i) {
        const bool use_topp = topp[i] > 0.f && topp[i] < 1.f;         // Sampler.java:88-98
        b->h_params[i] = SmpRow{temperature[i], topp[i], temperature[i] == 0.f ? 0.f : coins[i],
                                temperature[i] == 0.f ? SMP_GREEDY : use_topp ? SMP_TOPP : SMP_CATEGORICAL};
    }
    GL3_HIP(hipMemcpyAsync(b->params, b->h_params, (size_t)n * sizeof(SmpRow), hipMemcpyHostToDevice, ctx->stream));
    return GL3_OK;
}

static void bsample_enqueue(gl3_ctx* ctx, const float* logits, const int32_t* greedy, int n, bool any_topp) {
    gl3_bsample_state* b = ctx->bs;
    hipStream_t s = ctx->stream;
    const int v = ctx->d.vocab, nb = (v + RS_TILE - 1) / RS_TILE;
    const size_t smem = (size_t)(SM_CHUNK + 32) * 4 + ss_scratch_bytes(SM_CHUNK);
    int* n0 = b->res + 2 * b->rows;
    const dim3 ge(BSM_BLOCKS, n), gt(nb, n);
    hipLaunchKernelGGL(bsm_scale_max_kernel, ge, dim3(256), 0, s, logits, v, b->params, greedy, b->probs, b->aux, b->aux_stride, b->res, n0);
    hipLaunchKernelGGL(bsm_exp_kernel, ge, dim3(256), 0, s, b->probs, v, b->params, b->aux, b->aux_stride);
    hipLaunchKernelGGL(bsm_seqsum_kernel<false>, dim3(n), dim3(256), smem, s, b->probs, v, b->params, b->aux, b->aux_stride, b->res);
    hipLaunchKernelGGL(bsm_div_kernel, ge, dim3(256), 0, s, b->probs, v, b->params, b->aux, b->aux_stride);
    hipLaunchKernelGGL(bsm_seqsum_kernel<true>, dim3(n), dim3(256), smem, s, b->probs, v, b->params, b->aux, b->aux_stride, b->res);
    if (!any_topp) return;
    hipLaunchKernelGGL(btp_keys_kernel, ge, dim3(RS_THREADS), 0, s, b->probs, v, b->params, b->sort, b->sort_stride, n0);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(btp_hist_kernel, gt, dim3(RS_THREADS), 0, s, b->params, b->sort, b->sort_stride, v, pass, nb);
        hipLaunchKernelGGL(btp_scan_kernel, dim3(n), dim3(1024), 0, s, b->params, b->sort, b->sort_stride, v, 256 * nb);
        hipLaunchKernelGGL(btp_scatter_kernel, gt, dim3(RS_THREADS), 0, s, b->params, b->sort, b->sort_stride, v, pass, nb);
    }
    hipLaunchKernelGGL(btp_pick_kernel, dim3(n), dim3(256), smem, s, b->params, b->sort, b->sort_stride, v, n0, b->res);
}

int32_t gl3_sample_batch_finish(gl3_ctx* ctx, const float* logits_dev, const int32_t* greedy_dev, int32_t n, int32_t* tokens_out) {
    gl3_bsample_state* b = ctx->bs;
    hipStream_t s = ctx->stream;
    const int v = ctx->d.vocab;
    bool any_topp = false;
    for (int i = 0; i < n; ++i) any_topp |= b->h_params[i].mode == SMP_TOPP;
    static const bool graphs_off = getenv("GL3_NO_GRAPH") && atoi(getenv("GL3_NO_GRAPH"));
    if (!graphs_off && !gl3_roctx_on() && !(ctx->d.flags & GL3_FLAG_NO_GRAPH)) {
        if (b->graph_logits != logits_dev || b->graph_greedy != greedy_dev) {      // the step's logits buffer has grown: captured launches point at the old one
            bsample_drop_graphs(b);
            b->graph_logits = logits_dev; b->graph_greedy = greedy_dev;
        }
        const size_t slot = (size_t)2 * n + (any_topp ? 1 : 0);
        if (b->graphs.size() <= slot) b->graphs.resize(slot + 1, nullptr);
        if (!b->graphs[slot]) {
            hipGraph_t g = nullptr;
            GL3_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            bsample_enqueue(ctx, logits_dev, greedy_dev, n, any_topp);
            GL3_HIP(hipStreamEndCapture(s, &g));
            GL3_HIP(hipGraphInstantiate(&b->graphs[slot], g, nullptr, nullptr, 0));
            hipGraphDestroy(g);
        }
        GL3_HIP(hipGraphLaunch(b->graphs[slot], s));
    } else {
        bsample_enqueue(ctx, logits_dev, greedy_dev, n, any_topp);
    }
    GL3_HIP(hipGetLastError());
    GL3_HIP(hipMemcpyAsync(b->h_res, b->res, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    GL3_HIP(hipStreamSynchronize(s));
    int32_t r = gl3_tp_check(ctx);
    if (r != GL3_OK) return r;
    b->last_n = n;
    for (int i = 0; i < n; ++i) {
        const SmpRow& R = b->h_params[i];
        if (R.mode != SMP_TOPP || !b->h_res[2 * i + 1]) {
            tokens_out[i] = b->h_res[2 * i];
            if (R.mode == SMP_TOPP) ++ctx->topp_device;
            continue;
        }
        // a tie at the sampled rank of this row: the reference's heap history decides between equal probabilities — run it
        GL3_HIP(hipMemcpyAsync(b->h_probs, b->probs + (size_t)i * v, (size_t)v * 4, hipMemcpyDeviceToHost, s));
        GL3_HIP(hipStreamSynchronize(s));
        tokens_out[i] = topp_sample(b->h_probs, v, R.topp, R.coin, ctx->topp_indices);
        ++ctx->topp_host;
    }
    return GL3_OK;
}

int32_t gl3_sample_probs_row(gl3_ctx* ctx, int32_t row, float* out) {      // parity tap: what row `row` of the last batched sampled step was drawn from
    gl3_bsample_state* b = ctx->bs;
    if (!b || !b->last_n) GL3_FAIL(GL3_E_STATE, "no batched sampled step yet");
    if (row < 0 || row >= b->last_n) GL3_FAIL(GL3_E_ARG, "row outside the last batched sampled step");
    if (b->h_params[row].mode == SMP_GREEDY) GL3_FAIL(GL3_E_STATE, "the row was greedy: it has no probabilities");
    GL3_HIP(hipMemcpy(out, b->probs + (size_t)row * ctx->d.vocab, (size_t)ctx->d.vocab * 4, hipMemcpyDeviceToHost));
    return GL3_OK;
}
