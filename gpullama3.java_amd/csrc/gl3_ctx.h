// gl3_ctx.h — plan state shared by the translation units of libgpullama_hip.so.
// Mirrors what the reference keeps in State (J/inference/state/State.java:28-100) + TornadoWeights
// (J/inference/weights/tornado/TornadoWeights.java:20-48), but resident in HBM for the ctx lifetime.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gpullama3_hip.h"

// Slack behind every weight matrix (and the small-batch activation buffers): bdw_gemm_kernel's load rings run up to 16 tiles
// past the end of a strip instead of clamping or guarding their addresses (gl3_bd_gemm.h).
constexpr size_t GL3_TAIL_PAD = 256 * 1024;

// Internal format code of Q8_0 matrices run with an f32 activation (GL3_FLAG_F32_ACTIVATION): VL layout, gl3_veclane_kernels.h
// diagnostic switches: environment variable as a flag (unset / empty = default)
static inline bool env_flag(const char* name, bool dflt) {
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    return atoi(v) != 0;
}

// roctx ranges (SURVEY.md §5 "tracing"): GL3_ROCTX=1 brackets the decode step, every layer and every kernel class of an EAGER step
// (graphs are switched off: a replayed graph has no per-layer host calls) with roctxRangePush / Pop, resolved at run time from
// rocprofiler-sdk's roctx library (or roctracer's) so that the library has no link-time dependency on a profiler.
//     GL3_ROCTX=1 rocprofv3 --marker-trace --kernel-trace --output-format csv -- python bench.py --steps 1 --no-pp
#include <dlfcn.h>
struct Gl3Roctx { int (*push)(const char*) = nullptr; int (*pop)() = nullptr; };
static inline Gl3Roctx& gl3_roctx() {
    static Gl3Roctx r = [] {
        Gl3Roctx x;
        if (!env_flag("GL3_ROCTX", false)) return x;
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (h) {
            x.push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
            x.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (!x.push || !x.pop) x = Gl3Roctx{};
        }
        return x;
    }();
    return r;
}
static inline bool gl3_roctx_on() { return gl3_roctx().push != nullptr; }
struct Gl3Range {
    bool on;
    explicit Gl3Range(const char* name) : on(gl3_roctx_on()) { if (on) gl3_roctx().push(name); }
    Gl3Range(const char* what, int i) : on(gl3_roctx_on()) { if (on) { char b[48]; snprintf(b, sizeof b, "%s %d", what, i); gl3_roctx().push(b); } }
    ~Gl3Range() { if (on) gl3_roctx().pop(); }
    Gl3Range(const Gl3Range&) = delete;
    Gl3Range& operator=(const Gl3Range&) = delete;
};

constexpr int GL3_FMT_Q8V = 108;

struct Q8Mat {               // one repacked matrix: Q8T tiles (gl3_decode_kernels.h), VL groups (gl3_veclane_kernels.h) or row-lane groups
    uint8_t* w = nullptr;
    int rows = 0, k = 0;
    int ng = 0;              // Q8T: tile groups per strip = ceil(k/32 / 4)
    int nstrips = 0;         // Q8T: ceil(rows / 16)
    int fmt = 8;             // 8 = Q8_0 as Q8T tiles (int8 activation), 1 = F16, 2 = Q4_0, GL3_FMT_Q8V = Q8_0 with f32 activation
    bool vl = false;         // "VL" layout of the Vector-API-order kernels; false (F16 / Q4_0 only) = row-lane, scalar order
    size_t rl_group_bytes() const { return fmt == 1 ? (size_t)(k / 8) * 1024 : (size_t)(k / 32) * 1152; }
    size_t vl_group_bytes() const { return fmt == 1 ? (size_t)(k / 64) * 1024 : fmt == 2 ? (size_t)(k / 256) * 1152 : (size_t)(k / 128) * 1088; }
    size_t bytes() const {
        if (fmt != 8 && vl) return (size_t)((rows + 7) / 8) * vl_group_bytes();
        if (fmt != 8) return (size_t)((rows + 63) / 64) * rl_group_bytes();
        return (size_t)(nstrips + (nstrips & 1)) * ng * 2176;            // even #strips: the prefill GEMM reads 32-row groups
    }
    size_t algo_bytes() const {                                          // GGUF bytes (no padding)
        return (fmt == 8 || fmt == GL3_FMT_Q8V) ? (size_t)rows * (k / 32) * 34 : fmt == 1 ? (size_t)rows * k * 2 : (size_t)rows * (k / 32) * 18;
    }
};

struct gl3_layer {
    Q8Mat wqkv, wo, w1, w3, w2;
    float *attn_norm = nullptr, *ffn_norm = nullptr, *qnorm = nullptr, *knorm = nullptr;
    float *bq = nullptr, *bk = nullptr, *bv = nullptr;      // qwen2: this rank's rows of the q / k / v bias
    // qwen2moe: stacked routed experts ([n_experts * moe_hidden x dim] x 2, [n_experts * dim x moe_hidden]), the F32 router rows
    // [n_experts x dim] and the F32 shared-expert gate row [dim]; the shared expert itself is w1 / w3 / w2
    Q8Mat gate_exps, up_exps, down_exps;
    float *gate_inp = nullptr, *gate_inp_shexp = nullptr;
    uint32_t have = 0;       // bit per tensor id
};

// In-process tensor-parallel group (tests): ranks are host threads of one process sharing one device.  The ranks run the
// SAME peer-write gather kernel as separate processes do over xGMI; only the way a rank learns its peers' arena addresses
// differs (plain pointers here, hipIpcOpenMemHandle there).
struct gl3_local_group {
    int n = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0, generation = 0;
    std::vector<struct gl3_ctx*> ranks;
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const int gen = generation;
        if (++arrived == n) { arrived = 0; ++generation; cv.notify_all(); }
        else cv.wait(lk, [&] { return generation != gen; });
    }
};

constexpr int GL3_MAX_TP = 16;
enum { GL3_TP_NONE = 0, GL3_TP_RCCL = 1, GL3_TP_P2P = 2 };

// Tensor-parallel arena: ONE device allocation per rank that holds every gathered activation buffer plus the transport's
// header, at the same offsets on every rank, so a peer addresses "rank p's copy of buffer b" as peer_base[p] + off[b].
//   header: u32 flags[GL3_MAX_TP] (flags[p] = number of gathers rank p has pushed into this arena; written by the peers),
//           u32 seq (gathers completed by this rank), u32 arrive (workgroup ticket of the running gather kernel)
struct gl3_tp_arena {
    uint8_t* base = nullptr;
    size_t bytes = 0;                             // bytes this plan uses
    size_t cap = 0;                               // capacity of the allocation (>= bytes when it came from the pool)
    size_t off[8] = {};                           // byte offset of buffer GB_*; 0 = not allocated
    int pf_logits_rows = 0;                       // capacity of the batched-decode logits buffer (rows)
    int kind = 0;                                 // 0 uncached (default), 1 cached, 2 fine-grained, 3 uncached + hipFree (GL3_TP_ARENA experiments)
    bool pooled = false;                          // base goes back to the process-wide arena pool, not to hipFree (gl3_tp.hip)
};
constexpr size_t GL3_ARENA_HDR = 1024, GL3_ARENA_SEQ = 64, GL3_ARENA_ARRIVE = 68;      // bytes 256..511: checksums of GL3_TP_DEBUG (gl3_tp.hip)
// folded gathers (decode, Q8_0 int8 path): u32 flags[3][GL3_MAX_TP] per buffer GB_XB / GB_X / GB_HB (flags[b][p] = gathers of buffer b
// rank p has completed into this arena), u32 ticket[3] (finished producer wavefronts of the running launch), u32 step (decode steps)
constexpr size_t GL3_ARENA_FOLD = 512, GL3_ARENA_FOLD_TICKET = 704, GL3_ARENA_STEP = 720;

// Samplers (gl3_sample.hip).  A row's settings as the kernels read them from device memory.
enum { SMP_GREEDY = 0, SMP_CATEGORICAL = 1, SMP_TOPP = 2 };
struct SmpRow { float temperature, topp, coin; int mode; };
constexpr int GL3_DYN_ROW = 2, GL3_DYN_INTS = GL3_DYN_ROW + (int)(sizeof(SmpRow) / sizeof(int));     // layout of gl3_ctx::dyn / h_dyn

inline SmpRow gl3_smp_row(float temperature, float topp, float coin) {
    const bool use_topp = topp > 0.f && topp < 1.f;                   // Sampler.java:88-98
    return SmpRow{temperature, topp, temperature == 0.f ? 0.f : coin, temperature == 0.f ? SMP_GREEDY : use_topp ? SMP_TOPP : SMP_CATEGORICAL};
}

struct gl3_sample_state {
    int blocks;                                // workgroups per row of the element-wise launches (<= 256)
    bool graph;                                // replay the launches as one hipGraph per (rows, any top-p row) instead of launching eagerly
    int rows = 0;                              // capacity of every buffer below
    float* probs = nullptr;                    // [rows][vocab]
    float* aux = nullptr;                      // [rows][aux_stride]: `blocks` block maxima, the total, nchunks chunk ends
    int aux_stride = 0;
    uint32_t* sort = nullptr;                  // [rows][4 vocab + 256 nb]: (keys, indices) x 2, radix histogram
    size_t sort_stride = 0;
    int* res = nullptr;                        // [rows][2] {token, tie}, then [rows] n0 (top-p candidates)
    SmpRow* params = nullptr;                  // [rows] (the single-row entry's settings ride in gl3_ctx::dyn instead)
    SmpRow* h_params = nullptr;                // pinned
    int* h_res = nullptr;                      // pinned [rows][2]
    float* h_probs = nullptr;                  // pinned [vocab]: one tied row at a time
    std::vector<hipGraphExec_t> graphs;        // [2 n + (any top-p row)]
    const float* graph_logits = nullptr;       // the pointers the captured launches hold
    const int32_t* graph_greedy = nullptr;
    int last_n = 0;                            // rows of the last sampled step (their modes: h_params); 0 = no sampled step yet
    gl3_sample_state(int blocks_, bool graph_) : blocks(blocks_), graph(graph_) {}
};

// Token scores (score_rows_kernel, gl3_sample.hip): a row's settings as the kernel reads them, and everything scoring keeps on the device
struct ScoreRow { int target; float temperature; };
struct gl3_score_state {
    int rows = 0;                              // capacity of every buffer below
    ScoreRow* params = nullptr;                // [rows]
    ScoreRow* h_params = nullptr;              // pinned
    gl3_token_score* out = nullptr;            // [rows]
    gl3_token_score* h_out = nullptr;          // pinned
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // GL3_SCORE_TIMING=1 only
};

// Draft verification (verify_runs_kernel, gl3_sample.hip): a run and a row of the step as the kernel reads them.  A row's token is the
// draft of the row before it in its run; accept / emit are the caller's two coins of the row (not looked at on a greedy run).
// q (the _dist entries only; nothing else reads it): the slot of the draft table that holds the distribution the row's draft was drawn
// from, -1 = the draft is a fixed token (the one-hot rule).
struct VerifyRun { int row0, rows; float temperature; int pad; };
struct VerifyRow { int token; float accept, emit; int q; };
struct gl3_verify_state {
    int cap = 0;                               // rows (and so runs) every buffer below has room for: the plan's max_batch
    uint8_t* params = nullptr;                 // a step's VerifyRun[n_runs], then its VerifyRow[n]; room for cap of each
    uint8_t* h_params = nullptr;               // pinned, same layout
    gl3_verify_result* out = nullptr;          // [cap]
    gl3_verify_result* h_out = nullptr;        // pinned
};

// Draft distributions of a TARGET plan (gl3_draft_probs_put, gl3_sample.hip): slot s = the f32[vocab] distribution one drafted token was
// drawn from.  Allocated on the first put, freed with the sampler buffers.
struct gl3_draft_state {
    float* q = nullptr;                        // [max_batch][vocab]
    std::vector<uint8_t> written;              // [max_batch] the slot has been put
    hipEvent_t copied = nullptr;               // behind the last plan-to-plan copy: the draft plan's stream waits for it before it samples again
};

// Draft chain (gl3_forward_decode_chain, gl3_sample.hip): the ids the chained steps hand over and the coins they take, on the device.
// Allocated on the first chain for GL3_CHAIN_MAX entries, all or none, freed with the sampler buffers.
struct gl3_chain_state {
    int* ids = nullptr;                        // [GL3_CHAIN_MAX] id of step j, written by its hand-over launch
    float* coins = nullptr;                    // [GL3_CHAIN_MAX] coin of step j (step 0's also rides in dyn's SmpRow)
    int* h_ids = nullptr;                      // pinned
    float* h_coins = nullptr;                  // pinned
};

// Batched draft chain (gl3_forward_decode_batch_chain, gl3_sample.hip): the same lists for the n rows of a static-batched step, [step][row]
// with the call's row count as the stride, and what the hand-over launch needs to know of a row.  Allocated on the first batched chain for
// GL3_CHAIN_MAX * max_batch entries, all or none, freed with the sampler buffers.
struct gl3_batch_chain_state {
    int* ids = nullptr;                        // [k][n] id of row i at step j, written by the step's hand-over launch
    float* coins = nullptr;                    // [k][n] coin of row i at step j (0 for a greedy row)
    int* meta = nullptr;                       // [2][n]: steps of row i (k_i), first slot of row i in the target's table or -1
    int* h_ids = nullptr;                      // pinned
    float* h_coins = nullptr;                  // pinned
    int* h_meta = nullptr;                     // pinned
    bool sampled = false;                      // the running chain has a row at a temperature > 0: the coins are up and the rows' settings staged
};

struct gl3_ctx {
    gl3_model_desc d{};
    // derived (local = this tensor-parallel rank's share)
    int q_dim = 0, kv_dim = 0, heads_l = 0, kv_heads_l = 0, q_dim_l = 0, kv_dim_l = 0, hidden_l = 0, vocab_l = 0, dim_l = 0;
    int n_tsplit = 1;        // ceil(ctx / 64) score tiles
    int attn_win = 0;        // floats of a softmax row kept in LDS by the long-context attention kernels (longer rows: windows)
    bool wo_replicated = false;   // tensor parallel: every rank holds all rows of Wo (3 gathers per layer instead of 4)
    int wo_rows = 0;              // rows of Wo held by this rank: dim (replicated) or dim / tp
    // Granite (InferenceCore.forwardGranite): embedding / residual / logit multipliers (1 otherwise) and the score multiplier
    // (0 = divide by sqrt(head_size)); rope_arch = RoPE / per-head-norm flavour of the kernels (0 adjacent pairs, 1 qwen3, 2 NeoX)
    float emb_scale = 1.f, resid_scale = 1.f, logit_scale = 1.f, att_mul = 0.f;
    int rope_arch = 0;
    hipStream_t stream = nullptr;
    // weights
    Q8Mat emb, wcls;
    bool wcls_owned = false;
    float* out_norm = nullptr;
    uint32_t have_global = 0;
    std::vector<gl3_layer> layers;
    float *rope_cr = nullptr, *rope_ci = nullptr;
    uint64_t rope_n = 0;
    // state
    float *kcache = nullptr, *vcache = nullptr;   // [n_seqs][L][ctx][kv_dim_l]
    int n_seqs = 1;
    size_t kv_seq_stride = 0;                     // floats per sequence
    int* kv_copy_dst = nullptr;                   // [n_seqs] destination list of gl3_kv_seq_copy (n_seqs > 1 only)
    float *x = nullptr, *qkv = nullptr, *xb = nullptr, *hb = nullptr, *logits = nullptr, *att = nullptr;
    float *att_t = nullptr, *att_tmax = nullptr, *att_sums = nullptr;   // long-context decode: softmax numerators in attn_pv_kernel's operand order, per-tile score maxima, denominators
    float* xn = nullptr;                          // RMS-normalised activation (F16 / Q4_0 path only)
    float* taps = nullptr;                        // [L][dim] when GL3_FLAG_LAYER_TAPS
    // qwen2moe scratch (Qwen2MoEState.java:15-32): router logits [n_experts], routing weights [topk + 1] (last = shared-expert
    // gate), selected expert ids [topk], the selected experts' SwiGLU outputs [topk][moe_hidden], the down-projected outputs
    // [topk + 1][dim] (last = shared expert)
    float *moe_logits = nullptr, *moe_w = nullptr, *moe_hb = nullptr, *moe_y = nullptr;
    int* moe_sel = nullptr;                       // [topk] expert ids, then the router kernel's arrival ticket
    void* moe_slots = nullptr;                    // MoeSlots[n_layers][3]: gate/up with the shared expert merged, gate/up alone, down
    int *dyn = nullptr, *argmax = nullptr;        // dyn[0] = token, dyn[1] = position, then the SmpRow of a single-row sampled step (GL3_DYN_ROW)
    int* h_dyn = nullptr;                         // pinned, same layout
    const int* dyn_cur = nullptr;                 // (token, position) pair the next launches read: dyn, or an entry of dyn_seq
    int* dyn_seq = nullptr;                       // [2 * dyn_seq_cap] pairs of a sequential (token-by-token) prefill chunk
    int dyn_seq_cap = 0;
    float* h_logits = nullptr;                    // pinned f32[vocab]
    int* h_argmax = nullptr;
    int64_t topp_device = 0, topp_host = 0;       // top-p draws answered on the device / by the host heap (gl3_get_topp_counts)
    std::vector<int> topp_indices;
    // samplers (gl3_sample.hip): one set of kernels, one state per entry, so each entry's parity tap answers for its own last step
    gl3_sample_state smp_one{256, false};         // gl3_forward_decode_sample: one row, eager launches
    gl3_sample_state smp_rows{64, true};          // static-batched entries: grows with the batch, one hipGraph per (rows, any top-p row)
    gl3_score_state score;                        // gl3_forward_batch_score / gl3_score_rows
    gl3_verify_state verify;                      // gl3_forward_batch_verify / gl3_verify_rows and their _dist forms
    gl3_draft_state draft;                        // the draft distributions the _dist forms read
    gl3_chain_state chain;                        // gl3_forward_decode_chain
    gl3_batch_chain_state bchain;                 // gl3_forward_decode_batch_chain
    int last_sample_mode = -1;                    // SMP_* of the last gl3_forward_decode_sample or chained step (-1: none yet): what gl3_draft_probs_put may copy
    std::vector<std::pair<void*, size_t>> pinned;     // caller buffers registered with gl3_pin_host_buffer (logits land there directly)
    // upload staging
    uint8_t* staging = nullptr;
    size_t staging_bytes = 0;
    // batched prefill (gl3_prefill.hip)
    struct gl3_prefill_state* pf = nullptr;
    // execution
    bool finalized = false;
    // decode step incl. logits, one capture per attention regime (AttnRegime, gl3_decode_attn.h): [ATT_LONG] exists whenever graphs are
    // on and is correct at every position, [ATT_SHORT] (pos < AF_MAXN) and [ATT_MID] (pos < attn_mid) where the plan has the regime
    hipGraph_t graph[3] = {};
    hipGraphExec_t graph_exec[3] = {};
    int attn_mid = 0;                             // see attn_regime (gl3_decode_attn.h)
    bool fused_attn_ok = false;                   // shape admits attn_head_kernel (one launch per layer for positions < AF_MAXN)
    ncclComm_t comm = nullptr;
    gl3_local_group* lgrp = nullptr;
    bool use_rccl = false;                        // tensor-parallel gathers are active (any transport)
    int transport = GL3_TP_NONE;                  // GL3_TP_RCCL (gl3_tp_init) or GL3_TP_P2P (gl3_tp_p2p_attach / gl3_tp_attach_local)
    gl3_tp_arena arena;
    uint8_t* peer_base[GL3_MAX_TP] = {};          // arena of every rank as mapped into this process (peer_base[tp_rank] = arena.base)
    void* ipc_opened[GL3_MAX_TP] = {};            // mappings to close (hipIpcCloseMemHandle)
    int tp_fold_mask = 0;                         // TF_* consumers that wait in their own prologue
    bool tp_quiet = false;                        // gl3_profile_kernel: launch without the folded hand-overs (no pushes into the peers' arenas)
    int tp_fold = 0;                              // decode gathers folded into producers / consumers (gl3_api.hip tp_fold_setup): 0, 1, 2
    void* tp_recs = nullptr;                      // device TpRec[n_layers * 8 + 2]
    uint32_t* h_tp_err = nullptr;                 // pinned, device-visible: set by a gather kernel whose peers never arrived
    size_t tp_dbg_prev_off = 0, tp_dbg_prev_n4 = 0;   // GL3_TP_DEBUG: the previous gather of this forward call (re-checked by the next one)
    std::vector<hipEvent_t> ev;
    hipEvent_t prof_ev0 = nullptr, prof_ev1 = nullptr;   // non-null: the next matvec launch carries them as start / stop events
    // metrics
    double plan_ms = 0, copy_in_ms = 0;
    std::string err;
};

#define GL3_HIP(call)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                              \
            return e_ == hipErrorOutOfMemory ? GL3_E_OOM : GL3_E_HIP;                                  \
        }                                                                                              \
    } while (0)

#define GL3_NCCL(call)                                                                                 \
    do {                                                                                               \
        ncclResult_t r_ = (call);                                                                      \
        if (r_ != ncclSuccess) {                                                                       \
            ctx->err = std::string(#call) + ": " + ncclGetErrorString(r_);                             \
            return GL3_E_RCCL;                                                                         \
        }                                                                                              \
    } while (0)

#define GL3_FAIL(code, msg)                                                                            \
    do {                                                                                               \
        ctx->err = (msg);                                                                              \
        return (code);                                                                                 \
    } while (0)

// gl3_api.hip: in-place all-gather of buf = [tp][count_per_rank] over the plan's transport (RCCL or the local test group);
// which = GB_* id of the buffer (the local transport resolves the peers' pointers through gl3_gather_buf)
enum { GB_XB = 0, GB_X = 1, GB_HB = 2, GB_LOGITS = 3, GB_PF_X = 4, GB_PF_AO = 5, GB_PF_HB = 6, GB_PF_LOGITS = 7 };
float* gl3_gather_buf(gl3_ctx* c, int which);
int32_t gl3_all_gather(gl3_ctx* ctx, int which, size_t count_per_rank);
int32_t gl3_tp_arena_alloc(gl3_ctx* ctx);
void gl3_tp_arena_free(gl3_ctx* ctx);
int32_t gl3_tp_local_resolve(gl3_ctx* ctx);
int32_t gl3_tp_check(gl3_ctx* ctx);      // after a stream sync: GL3_E_RCCL if a gather timed out
namespace gl3 { struct AttnArgs; }       // gl3_decode_attn.h
// gl3_api.hip: the part of AttnArgs that layer l decides (its caches, rope tables, norms, biases, head counts and dimensions, eps,
// arch, att_mul); the caller adds the buffers, strides and window of its own launch
void gl3_attn_layer_args(const gl3_ctx* ctx, int l, gl3::AttnArgs& a);

// gl3_sample.hip
// single row: the launches behind a decode step whose set_dyn uploaded the row's settings, 8 bytes back
int32_t gl3_sample_run(gl3_ctx* ctx, const float* logits_dev, int32_t* token_out);
int32_t gl3_sample_probs(gl3_ctx* ctx, float* out);
void gl3_sample_free(gl3_ctx* ctx);
// row-batched entries: prepare = check + stage the per-row settings (before the step is enqueued), finish = the
// sampler's launches behind the step on the plan's stream, 8 * n bytes back, host heap for rows whose sampled rank is tied
int32_t gl3_sample_batch_prepare(gl3_ctx* ctx, int32_t n, const float* temperature, const float* topp, const float* coins, bool* all_greedy);
int32_t gl3_sample_batch_finish(gl3_ctx* ctx, const float* logits_dev, const int32_t* greedy_dev, int32_t n, int32_t* tokens_out);
int32_t gl3_sample_probs_row(gl3_ctx* ctx, int32_t row, float* out);
// token scores: prepare = every check + stage (target, temperature) of the n rows (temperature NULL: 1), before the step is enqueued;
// finish = score_rows_kernel behind the step on the plan's stream, 16 * n bytes back
int32_t gl3_score_prepare(gl3_ctx* ctx, int32_t n, const int32_t* targets, const float* temperature);
int32_t gl3_score_finish(gl3_ctx* ctx, const float* logits_dev, int32_t n, gl3_token_score* scores_out);
void gl3_score_free(gl3_ctx* ctx);
// draft verification: prepare = every check on (temperature, coins, q_slots) + stage the runs and rows (before the step is enqueued):
// tokens / coins ([n][2] or NULL) / q_slots by row, run_row0 / run_rows / temperature (NULL: greedy everywhere) by run; dist = the _dist
// entries (q_slots must be there; the others pass NULL); enqueue = verify_runs_kernel<dist> and the copy of 8 * n_runs bytes behind the
// step on the plan's stream; collect = wait and hand the records out
int32_t gl3_verify_prepare(gl3_ctx* ctx, int32_t n, const int32_t* tokens, const float* coins, int32_t n_runs, const int32_t* run_row0,
                           const int32_t* run_rows, const float* temperature, bool dist = false, const int32_t* q_slots = nullptr);
int32_t gl3_verify_enqueue(gl3_ctx* ctx, const float* logits_dev, const int32_t* greedy_dev, int32_t n_runs, bool dist = false);
int32_t gl3_verify_collect(gl3_ctx* ctx, int32_t n_runs, gl3_verify_result* results_out);
void gl3_verify_free(gl3_ctx* ctx);
// draft distributions of a target plan (the argument checks are gl3_api.hip's): one slot from the draft plan's last sampled row, from
// host memory, and back to the host
int32_t gl3_draft_put(gl3_ctx* ctx, int32_t slot, gl3_ctx* draft);
int32_t gl3_draft_put_host(gl3_ctx* ctx, int32_t slot, const float* q);
int32_t gl3_draft_get(gl3_ctx* ctx, int32_t slot, float* out);
// draft chain (the argument checks are gl3_api.hip's): prepare = the lists, the single-row sampler buffers (coins != NULL: a sampled chain)
// and the target's table on first use, then the k coins up in one copy; sample = the single-row sampler's launches behind a chained step;
// handover = the launch that passes step j's id (and its probabilities row, q_row != NULL) on; collect = the one wait, 4 * k bytes back
int32_t gl3_chain_prepare(gl3_ctx* ctx, int32_t k, const float* coins, gl3_ctx* target, int32_t slot0, float** q_row0);
int32_t gl3_chain_sample(gl3_ctx* ctx);
int32_t gl3_chain_handover(gl3_ctx* ctx, int32_t j, int32_t k, int32_t next_pos, bool sampled, float* q_row);
int32_t gl3_chain_collect(gl3_ctx* ctx, int32_t k, bool sampled, gl3_ctx* target, int32_t slot0, int32_t* tokens_out);
// one slot from row `row` of the draft plan's last batched sampled step (the argument checks are gl3_api.hip's)
int32_t gl3_draft_put_row(gl3_ctx* ctx, int32_t slot, gl3_ctx* draft, int32_t row);
// batched draft chain (the argument checks are gl3_api.hip's): prepare = the lists, the batched sampler's buffers and the rows' settings
// with the step-0 coins (any sampled row), the target's table on first use, then the [k][n] coins and the rows' (k_i, slot) up;
// sample = the batched sampler's launches behind a chained step of nj rows; handover = the launch that passes step j's ids (and the rows
// with a slot) on, id_src = {token, tie} pairs of the sampler (sampled_step) or the step's greedy ids; collect = the one wait, 4 * k * n
// bytes back, -1 where a row has no step, and the sampler state of the last single call
int32_t gl3_batch_chain_prepare(gl3_ctx* ctx, int32_t n, int32_t k, const int32_t* k_rows, const float* temperature, const float* coins, gl3_ctx* target,
                                const int32_t* slots);
int32_t gl3_batch_chain_sample(gl3_ctx* ctx, const float* logits_dev, const int32_t* greedy_dev, int32_t nj);
int32_t gl3_batch_chain_handover(gl3_ctx* ctx, int32_t j, int32_t n, int32_t nj, bool sampled_step, const int32_t* greedy_dev, int32_t* tokens_dev,
                                 int32_t* positions_dev, gl3_ctx* target);
int32_t gl3_batch_chain_collect(gl3_ctx* ctx, int32_t n, int32_t k, const int32_t* k_rows, const float* temperature, gl3_ctx* target, const int32_t* slots,
                                int32_t* tokens_out);

// gl3_prefill.hip
float* gl3_prefill_buf(gl3_ctx* ctx, int which);
int32_t gl3_prefill_alloc(gl3_ctx* ctx);
size_t gl3_prefill_norm_smem(int k);      // dynamic LDS of the batched RMSNorm + quantise launch for rows of k elements
void gl3_prefill_free(gl3_ctx* ctx);
int32_t gl3_prefill_moe_tap(gl3_ctx* ctx, int which, float* out, uint64_t n);      // gl3_get_buffer 9 / 10
int32_t gl3_prefill_run(gl3_ctx* ctx, int32_t seq, const int32_t* tokens, int32_t n, int32_t start_pos);
int32_t gl3_prefill_profile(gl3_ctx* ctx, int klass, int n, int iters, double* out_us, uint64_t* int8_ops);
int32_t gl3_decode_batch_run(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions, int32_t n,
                             float* logits_out, int32_t* argmax_out, bool finish = true);      // finish = false: enqueue only
// its two halves (a chain of steps stages once): the triples up; one step of n rows whose deepest row is at max_pos; and where the inputs live
int32_t gl3_decode_batch_stage(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions, int32_t n);
int32_t gl3_decode_batch_enqueue(gl3_ctx* ctx, int32_t n, int32_t max_pos);
void gl3_decode_batch_inputs(gl3_ctx* ctx, int32_t** tokens, int32_t** positions);
namespace gl3 { struct BatchPlan; }      // gl3_batch_plan.h
// one mixed step (gl3_forward_batch) whose plan the caller built and checked; outputs: the plan's out_rows, compact
int32_t gl3_batch_run(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions, int32_t n, const gl3::BatchPlan& bp,
                      float* logits_out, int32_t* argmax_out, bool finish = true);
int32_t gl3_prefill_tap_x(gl3_ctx* ctx, int row, int n);
int32_t gl3_prefill_attn_rows(gl3_ctx* ctx, int32_t out[4]);      // gl3_get_attn_rows
void gl3_decode_batch_outputs(gl3_ctx* ctx, const float** logits, const int32_t** greedy);
int32_t gl3_decode_batch_load_logits(gl3_ctx* ctx, const float* logits, int32_t n);
