/*
 * gpullama3_hip.h — C-ABI of libgpullama_hip.so, the MI355X-native replacement for the
 * TornadoVM TaskGraph layer of beehive-lab/GPULlama3.java.
 *
 * What it replaces (all paths relative to /root/reference/src/main/java/org/beehive/gpullama3/, "J/"):
 *   interface TornadoVMMasterPlan          J/tornadovm/TornadoVMMasterPlan.java:30-85
 *     initializeTornadoVMPlan(state,model) :55-70   -> gl3_create + gl3_upload_* + gl3_finalize
 *     forceCopyInReadOnlyData()            :79      -> gl3_finalize
 *     tornadoVMForwardDecode(position)     :81      -> gl3_forward_decode
 *     freeTornadoExecutionPlan()           :84      -> gl3_destroy
 *   TornadoVMMasterPlanBatchPrefillDecode.tornadoVMForwardBatchPrefill()
 *                                          J/tornadovm/TornadoVMMasterPlanBatchPrefillDecode.java:107-123
 *                                                   -> gl3_forward_prefill
 *   TornadoVMMasterPlanPrefillDecode.tornadoVMForwardPrefill(position)
 *                                          J/tornadovm/TornadoVMMasterPlanPrefillDecode.java:116
 *                                                   -> gl3_forward_prefill(n = 1)
 * No counterpart in the reference (one sequence per plan): the sequence slots (n_seqs), the batched steps and gl3_kv_seq_copy (prefix fork).
 * In the reference, inputs cross this seam by side effect through the shared State object
 * (J/inference/state/State.java:28-100: embeddingX, wrapXBatch, batchStartPosHolder, wrapLogits) and
 * TornadoWeights (J/inference/weights/tornado/TornadoWeights.java:20-48).  Here every argument is
 * explicit: token ids in, logits (or the greedy argmax, Sampler.java:21-28) out; the embedding row
 * gather that InferenceCore.forwardTornadoVM does on the host (J/inference/InferenceCore.java:956-980)
 * happens on the device.
 *
 * Ownership: the library owns all device memory for the ctx lifetime.  Every host pointer passed in
 * stays owned by the caller and only has to be valid during the call (weights: the caller's mmap'd
 * GGUF tensor-data segment, J/tensor/GGUF.java:105-137; raw ggml block layout, J/tensor/GGMLType.java:5-21).
 * Errors: every function returns a gl3_status (0 = OK, negative = error); no C++ exception crosses
 * the ABI; gl3_last_error() gives the message (the Java shim maps non-zero to RuntimeException, as the
 * reference throws UnsupportedOperationException / TornadoOutOfMemoryException —
 * J/tornadovm/plan/ForwardPlanFactory.java:84-86).
 * Threading: a gl3_ctx is not re-entrant but may be called from any thread, never concurrently
 * (the reference serialises inference with a lock, J/server/InferenceService.java:59).  forward_*
 * return only after the requested outputs are in host memory.
 */
#ifndef GPULLAMA3_HIP_H
#define GPULLAMA3_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GL3_API __attribute__((visibility("default")))

typedef struct gl3_ctx gl3_ctx;

typedef enum {
    GL3_OK = 0,
    GL3_E_ARG = -1,          /* bad argument / tensor shape mismatch */
    GL3_E_UNSUPPORTED = -2,  /* model x quantisation x mode not implemented (ForwardPlanFactory.java:80-121) */
    GL3_E_OOM = -3,          /* hipMalloc failed (TornadoOutOfMemoryException) */
    GL3_E_HIP = -4,          /* any other HIP runtime error */
    GL3_E_RCCL = -5,         /* collective failed */
    GL3_E_STATE = -6         /* call order violated (e.g. forward before finalize) */
} gl3_status;

/* model families with all three plan modes in the reference (ForwardPlanFactory.java:123-141) */
/* LLAMA: InferenceCore.forwardJava (also Mistral GGUFs, architecture "llama") and forwardJavaDevstral :178-261 (Devstral 2,
 * architecture "mistral3": the same graph with head_size = attention.key_length != dim / n_heads and a YaRN RoPE table); QWEN3: forwardJavaQwen3 (per-head q/k RMSNorm,
 * NeoX RoPE); QWEN2: forwardJavaQwen2 :434-563 (q/k/v bias, NeoX RoPE; Qwen2.5, DeepSeek-R1-Distill-Qwen). */
enum { GL3_ARCH_LLAMA = 0, GL3_ARCH_QWEN3 = 1, GL3_ARCH_QWEN2 = 2,
       GL3_ARCH_GRANITE = 3, /* InferenceCore.forwardGranite :814-924: the Llama graph + embedding / attention / residual / logit scalars */
       GL3_ARCH_PHI3 = 4,    /* InferenceCore.forwardJavaPhi3 :699-800: fused attn_qkv and gate|up tensors (GL3_T_WQKV, GL3_T_W13), NeoX RoPE */
       GL3_ARCH_QWEN2MOE = 5 /* InferenceCore.forwardJavaQwen2MoE :263-422 (Qwen1.5-MoE / Qwen2-MoE): the Qwen2 attention; the FFN is an F32
                              * router over n_experts (softmax over all, top n_experts_used by strict >, no renormalisation), the
                              * selected experts' SwiGLU FFNs accumulated into x in selection order, then the always-on shared
                              * expert scaled by sigmoid(ffn_gate_inp_shexp . xb).  Q8_0 matrices with the int8 activation, one rank.  max_batch > 1:
                              * batched prefill and static-batched decode (n_seqs > 1), the routed experts as one grouped GEMM over
                              * the step's (token, choice) assignments sorted by expert; max_batch <= 1: one sequence, a prefill
                              * chunk runs token by token. */ };

/* ggml tensor types of the wire format (J/tensor/GGMLType.java:5-21) */
enum { GL3_TYPE_F32 = 0, GL3_TYPE_F16 = 1, GL3_TYPE_Q4_0 = 2, GL3_TYPE_Q8_0 = 8,
       GL3_TYPE_Q4_K = 12, GL3_TYPE_Q5_K = 13, GL3_TYPE_Q6_K = 14 };   /* K-quants: converted to Q8_0 at load (gl3_kquant_to_q8_0) */

/* weight set (J/inference/weights/tornado/TornadoWeights.java:20-48; GGUF names in
 * J/model/loader/LlamaModelLoader.java:83-98, Qwen3ModelLoader.java:96-118) */
enum {
    GL3_T_TOKEN_EMBD = 0,   /* token_embd.weight        [vocab x dim]  quantised */
    GL3_T_OUTPUT_NORM = 1,  /* output_norm.weight       [dim]          F32       */
    GL3_T_OUTPUT = 2,       /* output.weight (wcls)     [vocab x dim]  quantised; omit when tied */
    GL3_T_ATTN_NORM = 3,    /* blk.L.attn_norm.weight   [dim]          F32       */
    GL3_T_WQ = 4,           /* blk.L.attn_q.weight      [qDim x dim]             */
    GL3_T_WK = 5,           /* blk.L.attn_k.weight      [kvDim x dim]            */
    GL3_T_WV = 6,           /* blk.L.attn_v.weight      [kvDim x dim]            */
    GL3_T_WO = 7,           /* blk.L.attn_output.weight [dim x qDim]             */
    GL3_T_FFN_NORM = 8,     /* blk.L.ffn_norm.weight    [dim]          F32       */
    GL3_T_W1 = 9,           /* blk.L.ffn_gate.weight    [hidden x dim]           */
    GL3_T_W2 = 10,          /* blk.L.ffn_down.weight    [dim x hidden]           */
    GL3_T_W3 = 11,          /* blk.L.ffn_up.weight      [hidden x dim]           */
    GL3_T_ATTN_Q_NORM = 12, /* blk.L.attn_q_norm.weight [head_size]    F32, qwen3 */
    GL3_T_ATTN_K_NORM = 13, /* blk.L.attn_k_norm.weight [head_size]    F32, qwen3 */
    GL3_T_BQ = 14,          /* blk.L.attn_q.bias        [q_dim]        F32, qwen2 (Qwen2StandardWeights q_bias) */
    GL3_T_BK = 15,          /* blk.L.attn_k.bias        [kv_dim]       F32, qwen2 */
    GL3_T_BV = 16,          /* blk.L.attn_v.bias        [kv_dim]       F32, qwen2 */
    GL3_T_WQKV = 17,        /* blk.L.attn_qkv.weight    [(qDim + 2 kvDim) x dim]  phi3: rows q | k | v (Phi3ModelLoader.java:112)          */
    GL3_T_W13 = 18,         /* blk.L.ffn_up.weight      [2 hidden x dim]          phi3: rows gate | up (forwardJavaPhi3 :778-780)          */
    /* qwen2moe (Qwen2MoEModelLoader.java:97-105).  The shared expert's ffn_{gate,up,down}_shexp.weight are uploaded as
     * GL3_T_W1 / GL3_T_W3 / GL3_T_W2 with gl3_model_desc.hidden = qwen2moe.feed_forward_length (sharedExpertHiddenDim). */
    GL3_T_FFN_GATE_INP = 19,       /* blk.L.ffn_gate_inp.weight        [n_experts x dim]               F32 (router)            */
    GL3_T_FFN_GATE_EXPS = 20,      /* blk.L.ffn_gate_exps.weight       [n_experts x moe_hidden x dim]  stacked routed experts  */
    GL3_T_FFN_UP_EXPS = 21,        /* blk.L.ffn_up_exps.weight         [n_experts x moe_hidden x dim]                          */
    GL3_T_FFN_DOWN_EXPS = 22,      /* blk.L.ffn_down_exps.weight       [n_experts x dim x moe_hidden]                          */
    GL3_T_FFN_GATE_INP_SHEXP = 23, /* blk.L.ffn_gate_inp_shexp.weight  [dim]                           F32 (shared-expert gate) */
    GL3_T_COUNT = 24
};

/* gl3_model_desc.flags */
#define GL3_FLAG_NO_GRAPH   0x1u  /* launch the decode step kernel by kernel instead of one hipGraph replay */
#define GL3_FLAG_LAYER_TAPS 0x2u  /* keep x after every layer for gl3_get_layer_x (parity tap)            */
#define GL3_FLAG_FORCE_RCCL 0x4u  /* run the tensor-parallel gathers even when tp_size == 1 (test hook)     */
#define GL3_FLAG_SCALAR_DOT 0x8u  /* F16 / Q4_0 matrices: the reference's SCALAR dot order (-Dllama.VectorBitSize=0,
                                     FloatTensor.scalarDot) instead of its default Vector-API order with a 256-bit species
                                     (FP16FloatTensor.vectorDot / Q4_0FloatTensor.vectorDot: 8 fused accumulator lanes).  Q8_0 is
                                     not affected: dotQ8Activation is scalar in both modes. */
#define GL3_FLAG_F32_ACTIVATION 0x10u /* Q8_0 matrices: -Dllama.quantizeActivation=false — f32 activation x dequantised weights in the
                                       * Vector-API order of Q8_0FloatTensor.vectorDot (256-bit species) instead of the int8 activation */
/* The species of the Vector-API order = -Dllama.VectorBitSize, default VectorShape.preferredShape() of the JVM's host
 * (J/tensor/standard/FloatTensor.java:21): 256 on an AVX2 host (this library's default), 512 on AVX-512 (e.g. the EPYC 9575F of an
 * MI355X node), 128 on SSE / NEON.  Only F16 / Q4_0 matrices and Q8_0 with GL3_FLAG_F32_ACTIVATION depend on it (the Q8_0 int8 path is
 * scalar).  GL3_FLAG_VECTOR_512: F16 matrices in the 16-accumulator order of FP16FloatTensor.vectorDot — single-token decode,
 * batched prefill (max_batch > 1), n_seqs > 1, static-batched decode and the batched samplers are all available, on one rank only (tp_size > 1
 * is refused with GL3_E_UNSUPPORTED); Q4_0 / Q8_0-f32act plans are refused with GL3_E_UNSUPPORTED — the reference throws UnsupportedOperationException
 * for them (Q4_0FloatTensor.java:118-120, Q8_0FloatTensor.java:165-167; run such a JVM with -Dllama.VectorBitSize=256).
 * GL3_FLAG_VECTOR_128 (4 accumulators; two fmas per block for Q8_0 / Q4_0): restated in the oracles, refused here (GL3_E_UNSUPPORTED). */
#define GL3_FLAG_VECTOR_512 0x20u
#define GL3_FLAG_VECTOR_128 0x40u

/* Configuration (J/model/Configuration.java via LlamaModelLoader.java:47-63 / Qwen3ModelLoader.java:48-74)
 * plus the plan-selection knobs the reference reads from system properties
 * (llama.prefillBatchSize -> max_batch, TornadoVMMasterPlan.java:39-41). */
typedef struct {
    uint32_t struct_size;   /* sizeof(gl3_model_desc), for forward compatibility */
    int32_t arch;           /* GL3_ARCH_* */
    int32_t dim;            /* embedding_length */
    int32_t hidden;         /* feed_forward_length */
    int32_t n_layers;       /* block_count */
    int32_t n_heads;        /* attention.head_count */
    int32_t n_kv_heads;     /* attention.head_count_kv */
    int32_t head_size;      /* dim / n_heads (llama, phi3) or attention.key_length (qwen3); a multiple of 32 in 32 .. 256 */
    int32_t vocab;
    int32_t ctx;            /* context length = KV-cache rows per layer (no upper bound besides memory: f32 K and V rows) */
    float   rms_eps;        /* attention.layer_norm_rms_epsilon */
    int32_t weight_type;    /* GL3_TYPE_* of the matrices */
    int32_t max_batch;      /* largest prefill chunk (llama.prefillBatchSize); <= 1: no batched prefill buffers */
    int32_t device;         /* HIP device ordinal */
    int32_t tp_rank;        /* tensor-parallel rank of this process (0 when tp_size == 1) */
    int32_t tp_size;        /* tensor-parallel degree: heads / hidden units / dim rows of W2 / vocab rows are split tp_size ways
                             * (Wo is replicated: a rank computes the whole projection from the gathered attention output) */
    uint32_t flags;         /* GL3_FLAG_* */
    int32_t n_seqs;         /* independent sequences with their own KV cache (static batched decode); 0 or 1 = one */
    /* GL3_ARCH_GRANITE only (GraniteLoader.java:55-58: granite.embedding_scale, granite.attention.scale, granite.residual_scale,
     * granite.logit_scale): x *= embedding_scale after the embedding lookup, score *= attention_scale (instead of / sqrt(head_size)),
     * block output *= residual_scale before the residual add, logits *= logit_scale */
    float embedding_scale, attention_scale, residual_scale, logit_scale;
    /* GL3_ARCH_QWEN2MOE only (Qwen2MoEModelLoader.java:56-84: qwen2moe.expert_count, qwen2moe.expert_used_count, and the first
     * dimension of blk.0.ffn_down_exps.weight); 0 for every other architecture */
    int32_t n_experts, n_experts_used, moe_hidden;
} gl3_model_desc;

/* Per-kernel-class device time of one instrumented decode step (HIP events around every launch). */
enum { GL3_K_MATVEC_QKV = 0, GL3_K_MATVEC_WO = 1, GL3_K_MATVEC_GATEUP = 2, GL3_K_MATVEC_DOWN = 3,
       GL3_K_MATVEC_LOGITS = 4, GL3_K_ATTENTION = 5, GL3_K_OTHER = 6, GL3_K_COLLECTIVE = 7, GL3_K_COUNT = 8 };
typedef struct {
    double   ms[GL3_K_COUNT];        /* summed event-to-event time per class */
    uint32_t launches[GL3_K_COUNT];
    uint64_t bytes[GL3_K_COUNT];     /* algorithmic HBM bytes per class (weights + vectors), SURVEY.md §8d */
} gl3_kernel_times;

GL3_API const char* gl3_version(void);

/* Build the plan: allocates weights/KV/scratch in HBM (TornadoVMMasterPlan ctor: graph build + JIT are
 * replaced by precompiled gfx950 code objects). */
GL3_API int32_t gl3_create(const gl3_model_desc* desc, gl3_ctx** out);

/* Copy one tensor to HBM (FIRST_EXECUTION copy-in of the reference).  `host` is raw ggml blocks for the
 * FULL tensor, also under tensor parallelism (the library keeps only this rank's slice).  The library may
 * repack (split scale/quant planes); bytes moved per token are unchanged. */
GL3_API int32_t gl3_upload_tensor(gl3_ctx* ctx, int32_t tensor_id, int32_t layer, const void* host,
                                  uint64_t bytes, int32_t ggml_type);

/* freq_cis_real / freq_cis_imag as the host precomputes them (J/inference/operation/RoPE.java:6-37);
 * n = rows * head_size/2 floats, rows >= ctx. */
GL3_API int32_t gl3_upload_rope(gl3_ctx* ctx, const float* cr, const float* ci, uint64_t n);

/* Join a tensor-parallel group (one process per GPU; must precede gl3_finalize).  Two transports for the in-place
 * all-gathers of the row-split plan:
 *   peer-write over xGMI (default): every rank exports the IPC handle of its arena of gathered buffers
 *     (gl3_tp_p2p_handle, 64 bytes), the host exchanges the handles through any side channel (torch.distributed
 *     all_gather_object, a file, a socket) and hands all tp_size of them, in rank order, to gl3_tp_p2p_attach; one small
 *     kernel per gather then stores this rank's slice straight into the peers' buffers (csrc/gl3_tp.hip);
 *   RCCL (fall-back): `unique_id` is the id made by gl3_tp_unique_id on rank 0 and broadcast by the host. */
/* Transport choice BEFORE any plan exists: *reachable = how many of the n `peer_devices` (HIP ordinals) `device` can address
 * directly (hipDeviceCanAccessPeer; a device reaches itself).  reachable < n: use the RCCL transport (gl3_tp_init). */
GL3_API int32_t gl3_tp_peer_access(int32_t device, const int32_t* peer_devices, int32_t n, int32_t* reachable);
GL3_API int32_t gl3_tp_p2p_handle(gl3_ctx* ctx, void* out, uint64_t bytes);                  /* bytes >= 64 */
GL3_API int32_t gl3_tp_p2p_attach(gl3_ctx* ctx, const void* handles, uint64_t bytes);        /* tp_size x 64 bytes */
GL3_API int32_t gl3_tp_unique_id(void* out, uint64_t bytes);   /* bytes >= 128 */
GL3_API int32_t gl3_tp_init(gl3_ctx* ctx, const void* unique_id, uint64_t bytes);

/* In-process tensor-parallel group for TESTS on one GPU: `n` plans (one host thread each, same device) run the same
 * peer-write gather kernel, row split, kernel arguments and gather points as `n` processes on `n` GPUs; only the peers'
 * arena addresses are exchanged as plain pointers instead of IPC handles.  Create once, pass to every rank's
 * gl3_tp_attach_local before gl3_finalize (which waits for all ranks), destroy after the plans. */
typedef struct gl3_local_group gl3_local_group;
GL3_API int32_t gl3_local_group_create(int32_t n, gl3_local_group** out);
GL3_API void gl3_local_group_destroy(gl3_local_group* g);
GL3_API int32_t gl3_tp_attach_local(gl3_ctx* ctx, gl3_local_group* g);
/* After gl3_finalize: how this plan's decode step hands the gathered activations over (gl3_api.hip tp_fold_setup).  *mode = 0: one
 * gather launch per hand-over (every type but the Q8_0 int8 path, the RCCL transport, GL3_TP_FOLD=0); 1: the producing kernels
 * write their results into the peers' arenas themselves.  *consumer_mask: bit set = that consumer waits for the peers in its own
 * prologue (1 wo, 2 down, 4 qkv, 8 logits, 16 embedding; GL3_TP_FOLD=2 sets all), clear = a one-wavefront wait launch precedes it. */
GL3_API int32_t gl3_tp_fold_mode(gl3_ctx* ctx, int32_t* mode, int32_t* consumer_mask);
/* The per-rank arena is UNCACHED device memory and is never returned to the allocator when a plan is destroyed: it waits in a process-wide pool and
 * is re-used by the next tensor-parallel plan of the device that fits into it (best fit, capacity >= request), so a process retains at most as many
 * arenas as it had tensor-parallel plans alive at the same time.  gl3_tp_pool_stats reports what is retained (device -1: all devices);
 * gl3_tp_pool_trim releases it — only for a quiescent process (model reload in a server): freed uncached pages that come back from a later
 * hipMalloc under the cached policy were the root cause of stale activation rows (tensor parallelism). */
GL3_API int32_t gl3_tp_pool_stats(int32_t device, uint64_t* arenas, uint64_t* bytes);
GL3_API int32_t gl3_tp_pool_trim(int32_t device);

/* forceCopyInReadOnlyData(): checks that every tensor arrived, ties wcls to token_embd when
 * GL3_T_OUTPUT was not uploaded (AbstractModelLoader.java:194), captures the decode hipGraph. */
GL3_API int32_t gl3_finalize(gl3_ctx* ctx);

/* One decode step (InferenceCore.forwardTornadoVM + plan.tornadoVMForwardDecode(position)).
 * logits_out: caller-allocated f32[vocab] or NULL; argmax_out: first index of the maximum or NULL. */
GL3_API int32_t gl3_forward_decode(gl3_ctx* ctx, int32_t token, int32_t position, float* logits_out,
                                   int32_t* argmax_out);

/* One decode step + Sampler.selectSampler(vocab, temperature, topp, seed).sampleToken(logits)
 * (J/inference/sampler/Sampler.java:76-123): temperature == 0 -> greedy argmax; else logits / temperature, softmax (max,
 * exp in double, strictly sequential f32 sum, divide) on the device, then CategoricalSampler (topp outside (0,1); on the
 * device, 4 bytes come back) or ToppSampler (probabilities to the host, the reference's heap selection in native code).
 * `coin` is rng.nextFloat(1f) drawn by the CALLER from its own RandomGenerator — RandomGeneratorFactory.getDefault()
 * .create(seed) in the reference — one per sampled token, exactly where the reference draws it; the library holds no RNG, so
 * the random stream and the sampled ids are the reference's by construction. */
GL3_API int32_t gl3_forward_decode_sample(gl3_ctx* ctx, int32_t token, int32_t position, float temperature, float topp,
                                          float coin, int32_t* token_out);
/* Parity tap: the probabilities (f32[vocab]) the last gl3_forward_decode_sample sampled from. */
GL3_API int32_t gl3_get_sample_probs(gl3_ctx* ctx, float* out);
/* Parity / measurement tap: top-p draws of this plan answered by the device path (8 bytes back) and by the host heap (a tie between equal
 * probabilities at the sampled rank, or a cumulative sum that reaches the last three candidates, which the reference's heap does not emit in
 * sorted order: the reference's heap order decides, gl3_sample.hip). */
GL3_API int32_t gl3_get_topp_counts(gl3_ctx* ctx, int64_t* on_device, int64_t* on_host);

/* Optional: page-lock a caller-owned host buffer (e.g. the MemorySegment the Java shim passes as logits_out on every step) so
 * that gl3_forward_decode copies the logits straight into it instead of going through the plan's pinned staging buffer and a
 * host memcpy.  The buffer must stay allocated until gl3_unpin_host_buffer / gl3_destroy.  `ptr` and `bytes` must be multiples
 * of 4096: registration pins and maps whole pages, so the buffer has to own its pages (mmap / posix_memalign /
 * Arena.allocate(bytes, 4096) with the size rounded up); anything else returns GL3_E_ARG and the plan keeps staging. */
GL3_API int32_t gl3_pin_host_buffer(gl3_ctx* ctx, void* ptr, uint64_t bytes);
GL3_API int32_t gl3_unpin_host_buffer(gl3_ctx* ctx, void* ptr);

/* Batched prefill of tokens[0..n) at positions start_pos.. (no logits, as the reference skips them).
 * n <= max_batch. */
GL3_API int32_t gl3_forward_prefill(gl3_ctx* ctx, const int32_t* tokens, int32_t n, int32_t start_pos);

/* Same for sequence `seq` (0 <= seq < n_seqs); gl3_forward_prefill is seq = 0. */
GL3_API int32_t gl3_forward_prefill_seq(gl3_ctx* ctx, int32_t seq, const int32_t* tokens, int32_t n, int32_t start_pos);

/* Static batched decode (BASELINE.json config 5; announced for the reference as PR #129, README.md:74): one decode
 * step for n independent sequences: token tokens[i] of sequence seq_ids[i] at position positions[i].  The n matvecs
 * become one int8-MFMA GEMM over the shared weights (weights are streamed once per step).  n <= max_batch, distinct
 * seq_ids.  logits_out: f32[n][vocab] or NULL; argmax_out: int32[n] (greedy id per sequence, sampled on the device) or NULL. */
GL3_API int32_t gl3_forward_decode_batch(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions,
                                         int32_t n, float* logits_out, int32_t* argmax_out);

/* One static-batched decode step + Sampler.selectSampler(vocab, temperature[i], topp[i], .).sampleToken(logits row i) for every
 * row (gl3_forward_decode_sample, row by row).  temperature / topp / coins: f32[n], one entry per row (the requests of one batch
 * have their own settings); temperature[i] == 0 -> the greedy first-max id of row i (its coin is not looked at); otherwise
 * coins[i] = rng.nextFloat(1f) drawn by the CALLER from row i's own RandomGenerator, in [0, 1); 0 < topp[i] < 1 -> ToppSampler,
 * else CategoricalSampler.  tokens_out: int32[n]; 8 * n bytes come back, and only a top-p row whose sampled rank is shared by
 * equal probabilities, or whose cumulative sum does not exceed topp before the last three candidates, has its probabilities copied
 * out for the reference's heap (counted by gl3_get_topp_counts, one count per
 * non-greedy top-p row).  The number of sampler launches does not depend on n (gl3_sample.hip).  Everything else as
 * gl3_forward_decode_batch; with every temperature 0 the ids are its argmax_out.  Tensor parallel (tp_size > 1): every rank is called
 * with the same arguments (coins included), samples every row from the gathered, rank-chunked logits and returns the same ids; nothing
 * is communicated behind the logits gather.  GL3_E_UNSUPPORTED: max_batch <= 1; tp_size > 1 with n > 64 (the gathered logits hold
 * min(max_batch, 64) rows), refused before anything is staged. */
GL3_API int32_t gl3_forward_decode_batch_sample(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids,
                                                const int32_t* positions, int32_t n, const float* temperature,
                                                const float* topp, const float* coins, int32_t* tokens_out);
/* Mixed batched step: prompt chunks and decode rows of many sequences in one pass over the weights (continuous batching, speculative
 * verification, perplexity).  The n rows are a list of RUNS: a run is a maximal stretch of consecutive rows with the same seq_ids[i], at
 * consecutive ascending positions; a sequence id belongs to at most one run.  A run of one row is a decode row, a longer run a prompt
 * chunk that may start at any position.  A row sees its sequence's KV rows below its position — as earlier calls left them or as earlier
 * rows of its run write them in this step — plus its own, so its result is what gl3_forward_prefill_seq / gl3_forward_decode_batch give
 * for that token and position.  Output rows: the rows with want_logits[i] != 0, in row order (want_logits == NULL: the last row of every
 * run); logits_out: f32[n_out][vocab] or NULL, argmax_out: int32[n_out] or NULL.  n_out == 0 is a pure multi-sequence prefill (no output
 * norm, vocabulary projection or argmax is launched).  Afterwards gl3_get_x returns x of the last row and gl3_get_buffer(4..6) hold all n
 * rows in step order (after a step on tp_size > 1 ranks rank-chunked, [tp_size][n][cols / tp_size], as after a tensor-parallel prefill).  The step runs eagerly (its shape differs from call to call); a step whose runs are all single rows and whose rows
 * all want logits is a gl3_forward_decode_batch step.  Attention of a step with a run of several rows, at any depth: its 8-row tiles whose
 * score rows fit LDS run on the one-launch tiled kernels, its deeper rows on the long-context scores / softmax / weighted-sum kernels (both
 * in their run-table forms, the split by depth per tile, not per step); head sizes other than 32 / 64 / 128 and more than 4 query heads per
 * kv head run row by row (gl3_get_attn_rows tells).  GL3_E_ARG, before anything is enqueued: null arrays, n <= 0, n > max_batch, a
 * token / sequence / position out of range or a run ending past ctx, a sequence id in two runs, positions inside a run that are not
 * consecutive ascending.  Tensor parallel (tp_size > 1): every rank is called with the same arguments and returns the same outputs; the
 * layers and both attention forms run on the rank's heads and chunks, each rank projects its rows of the vocabulary, and the logits of
 * the output rows are gathered once per step.  GL3_E_UNSUPPORTED: max_batch <= 1; tp_size > 1 with more than 64 output rows in one
 * step (the gathered logits hold min(max_batch, 64) rows) — refused with the arguments, before anything is staged or enqueued; the step
 * itself may still have up to max_batch rows. */
GL3_API int32_t gl3_forward_batch(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions,
                                  const int8_t* want_logits, int32_t n, float* logits_out, int32_t* argmax_out);
/* The same step + the sampler of gl3_forward_decode_batch_sample over the output rows: temperature / topp / coins / tokens_out have one
 * entry per OUTPUT row (n_out > 0 with any of them NULL: GL3_E_ARG).  gl3_get_sample_probs_row (row = output row) and gl3_get_topp_counts
 * answer for it.  Tensor parallel: as gl3_forward_batch, and every rank samples every output row from the gathered logits with the
 * caller's coins, so all ranks return the same ids; GL3_E_UNSUPPORTED for more than 64 output rows, before the sampler stages anything. */
GL3_API int32_t gl3_forward_batch_sample(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions,
                                         const int8_t* want_logits, int32_t n, const float* temperature, const float* topp,
                                         const float* coins, int32_t* tokens_out);
/* What softmaxInPlace(logits row / temperature) (FloatTensor.java:203-219) says about ONE token of an output row, all f32 with the
 * reference's arithmetic: v[i] = l[i] / T, max = max_i v[i], e[i] = (float) exp((double) (v[i] - max)), sum = the strictly sequential sum
 * ((0f + e[0]) + e[1]) + ..., prob = e[target] / sum, logit = v[target].  prob underflows to 0 once logit - max is below about -103; a
 * caller that needs ln p computes (double) (logit - max) - log((double) sum). */
typedef struct { float prob, logit, max, sum; } gl3_token_score;
/* The step of gl3_forward_batch + the score of one known token per OUTPUT row (speculative verification at a temperature, perplexity):
 * targets: int32[n_out], the token whose probability is wanted (the next token of the text, the drafted token); temperature: f32[n_out],
 * each > 0, or NULL for 1 everywhere; scores_out: gl3_token_score[n_out]; argmax_out: int32[n_out] (the greedy id of every output row, as
 * gl3_forward_batch gives it) or NULL.  The logits never leave the device and no [rows][vocab] buffer beside them exists: one launch, one
 * workgroup per row, behind the step on the plan's stream, and 16 * n_out bytes come back in one copy (gl3_sample.hip).  n_out == 0 is a
 * pure prefill, as in gl3_forward_batch_sample.  GL3_E_ARG, before anything is enqueued: everything gl3_forward_batch refuses, n_out > 0
 * with targets or scores_out NULL, a target outside [0, vocab), a temperature that is not > 0 (NaN included).  Tensor parallel: as
 * gl3_forward_batch; every rank scores every output row from the gathered, rank-chunked logits and returns the same scores.
 * GL3_E_UNSUPPORTED: max_batch <= 1; tp_size > 1 with more than 64 output rows, before the scorer stages anything. */
GL3_API int32_t gl3_forward_batch_score(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions,
                                        const int8_t* want_logits, int32_t n, const int32_t* targets, const float* temperature,
                                        gl3_token_score* scores_out, int32_t* argmax_out);
/* Parity tap: the same scores on caller-supplied logits (host f32[n][vocab]); no forward pass, no KV change.  Needs a plan with
 * max_batch > 1; n <= max_batch (tp_size > 1: n <= 64).  The logits buffer of the batched step is overwritten: on tp_size > 1 ranks the
 * rows are laid out rank-chunked as a step leaves them, so the tap runs the reader a step runs; it needs no peer.  Errors as above. */
GL3_API int32_t gl3_score_rows(gl3_ctx* ctx, const float* logits, int32_t n, const int32_t* targets, const float* temperature,
                               gl3_token_score* scores_out);
/* Speculative decoding: the step of gl3_forward_batch over runs that carry DRAFTED tokens, and the decision, taken on the device, how many
 * drafts of every run stand and which token follows them.  The rows are the runs of gl3_forward_batch, with the same rules and the same
 * refusals; every row is an output row.  In a run of m rows with tokens t0 .. t(m-1), t0 is the sequence's last real token and t1 .. t(m-1)
 * are drafts: row i predicts the token after ti, so its draft is d = t(i+1); the last row has none.  results_out: one record per run, in run
 * order (*n_runs_out of them; room for n is always enough): accepted = a, the number of leading rows whose draft stands, token = the token
 * that follows them.  The sequence then continues with t1 .. ta, token.  8 * n_runs bytes come back in one copy; no logits leave the device.
 * temperature: f32[n_runs], or NULL for greedy everywhere.
 *   Greedy run (temperature 0): row i accepts iff its greedy id (the first index of the maximum, from the step's own greedy scan) equals d;
 *   token = the greedy id of row a.  The ids a caller collects this way are those of decoding one token per step.
 *   Sampled run (T > 0): coins: f32[n][2] drawn by the CALLER from the sequence's own generator, each in [0, 1) — coins[i][0] the accept
 *   coin of row i, coins[i][1] its emit coin (the library holds no RNG; coins of greedy runs are not looked at, and coins may be NULL when
 *   every run is greedy).  With p = softmaxInPlace(logits row / T) in the arithmetic of gl3_token_score (p[d] is bit for bit its prob), row
 *   i accepts iff coins[i][0] < p[d], strictly.  At the first rejecting row a: q = p with q[d] = 0f, S' = the strictly sequential f32 sum of
 *   q, r = coins[a][1] * S', token = the first j with r < cdf_j (cdf = the sequential f32 sum of q), or the largest index other than d if
 *   there is none.  If all m - 1 drafts stand, a = m - 1 and token is CategoricalSampler on row m - 1 with the coin coins[m-1][1]: what
 *   gl3_forward_batch_sample gives that row with topp = 0.  For a draft that is a fixed token this is the speculative-sampling rule with a
 *   one-hot draft distribution, lossless in distribution: P(first emitted = x) = p(d) [x = d] + (1 - p(d)) q(x) / S' = p(x).  There is no
 *   top-p here.
 * KV: the step writes the K / V rows of all m positions of a run that starts at position p.  The rows above position p + a belong to rejected
 * drafts; the caller's next run on that sequence starts at p + a + 1 and overwrites them before anything reads them, since a row sees the
 * rows below its position plus its own.  Nothing has to be rolled back.
 * The decision is one launch behind the step whatever n and the number of runs (gl3_sample.hip).  gl3_get_x and the step buffers answer as
 * after the gl3_forward_batch step over the same rows.  GL3_E_ARG, before anything is enqueued: everything gl3_forward_batch refuses, NULL
 * results_out or n_runs_out, a temperature that is negative or NaN, coins == NULL while some run has T > 0, a coin outside [0, 1) on a run
 * with T > 0.  GL3_E_UNSUPPORTED: max_batch <= 1; tp_size > 1 — draft verification (this entry and gl3_verify_rows) remains ONE-rank:
 * its kernel reads plain [n][vocab] logits.  Every rank answers so and enqueues nothing. */
typedef struct { int32_t accepted, token; } gl3_verify_result;
GL3_API int32_t gl3_forward_batch_verify(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions, int32_t n,
                                         const float* temperature, const float* coins, gl3_verify_result* results_out,
                                         int32_t* n_runs_out);
/* Parity tap: the same decision on caller-supplied logits (host f32[n][vocab]); no forward pass, no KV change.  run_rows: int32[n_runs], the
 * rows of every run, each >= 1, summing to n <= max_batch (the entry has no other row count: logits and tokens must hold that many rows);
 * tokens: int32[n], each inside the vocabulary.  The logits buffer of the batched
 * step is overwritten.  Otherwise errors as above. */
GL3_API int32_t gl3_verify_rows(gl3_ctx* ctx, const float* logits, const int32_t* tokens, const int32_t* run_rows, int32_t n_runs,
                                const float* temperature, const float* coins, gl3_verify_result* results_out);
/* Speculative decoding with a DRAFT MODEL: a second plan in the same process drafts with gl3_forward_decode_sample, and the target plan
 * verifies each draft against the distribution it was actually drawn from.  The target plan owns a device table q[max_batch][vocab] of f32,
 * allocated on the first put and freed with the plan; slot s holds the distribution ONE drafted token was drawn from.
 * gl3_draft_probs_put: slot `slot` of `target` = the row gl3_get_sample_probs(draft) would return, the softmax row of the draft plan's last
 * gl3_forward_decode_sample.  One device-to-device copy on the target's stream; the call returns once it is enqueued (the draft's forward has
 * returned, so the row is complete; the draft's stream is made to wait for the copy before it runs anything else, the host waits for
 * nothing).  GL3_E_ARG: a null plan, draft == target, slot outside [0, max_batch) of the target, different vocabularies, plans on different
 * devices.  GL3_E_STATE: the draft plan has sampled nothing yet; its last gl3_forward_decode_sample was greedy (temperature 0: there is no
 * row); it went through ToppSampler (0 < topp < 1: the row is the untruncated softmax, not what the token was drawn from, and verifying
 * against it would silently stop being lossless).  GL3_E_UNSUPPORTED: a target without max_batch > 1; tp_size > 1 on either plan. */
GL3_API int32_t gl3_draft_probs_put(gl3_ctx* target, int32_t slot, gl3_ctx* draft);
/* The same for a draft plan that drafts many sequences in static-batched steps: slot `slot` of `target` = the row
 * gl3_get_sample_probs_row(draft, row) would return, the softmax row of row `row` of the draft plan's last batched sampled step
 * (gl3_forward_decode_batch_sample, or the last step of a gl3_forward_decode_batch_chain) or gl3_sample_rows call.  One
 * device-to-device copy on the target's stream, ordered against the draft's stream as in gl3_draft_probs_put.  GL3_E_ARG: a null plan,
 * draft == target, slot outside [0, max_batch) of the target, row outside the rows of that step, different vocabularies, plans on different
 * devices.  GL3_E_STATE: no batched sampled step yet (or the last one was all greedy); the row was greedy; the row went through top-p.
 * GL3_E_UNSUPPORTED: a target without max_batch > 1; tp_size > 1 on either plan. */
GL3_API int32_t gl3_draft_probs_put_row(gl3_ctx* target, int32_t slot, gl3_ctx* draft, int32_t row);
/* Parity tap: the same slot from host memory, q: f32[vocab], taken as it is — finite and >= 0 is the caller's contract, nothing scans it. */
GL3_API int32_t gl3_draft_probs_put_host(gl3_ctx* target, int32_t slot, const float* q);
/* Parity tap: slot `slot` back to the host (out: f32[vocab]).  GL3_E_STATE for a slot that was never written. */
GL3_API int32_t gl3_get_draft_probs(gl3_ctx* target, int32_t slot, float* out);
/* gl3_forward_batch_verify with a draft distribution per row.  Everything — runs, coins [n][2], the KV contract, one decision launch, 8 bytes
 * per run back, the refusals — is gl3_forward_batch_verify's; the addition is q_slots: int32[n], one entry per row.  For a row i that has a
 * draft d (every row of a run but its last): q_slots[i] = -1 -> the row is decided by gl3_forward_batch_verify's one-hot rule, bit for bit;
 * q_slots[i] = s >= 0 -> by the rule below with q = slot s of the draft table.  Greedy runs (temperature 0) and the last row of a run never
 * look at their entry.
 *   All in f32, p exactly as in gl3_forward_batch_verify (p[j] = e[j] / sum, gl3_token_score's arithmetic).
 *   Accept iff coins[i][0] * q[d] < p[d]: one f32 product, strictly less, no division — min(1, p[d] / q[d]) without the quotient; q[d] == 0
 *   accepts iff p[d] > 0.
 *   Reject: r[j] = fmaxf(p[j] - q[j], 0f) for every j.  A rejection implies q[d] >= p[d], so r[d] == 0 and d cannot come back; nothing
 *   special-cases it.  S' = the strictly sequential f32 sum of r, target = coins[i][1] * S', token = the first j with target < cdf_j (cdf =
 *   the sequential f32 sum of r).  No such j and S' > 0 (the product rounded up to S'): the largest j with r[j] > 0.  S' == 0 (p <= q
 *   everywhere, e.g. q bitwise equal to p): the row's greedy id, from the step's own greedy scan.
 *   All drafts of a run stand: the last row is CategoricalSampler with its emit coin, unchanged.
 *   Lossless in distribution for a draft d drawn from q: P(first emitted = x) = q(x) min(1, p(x) / q(x)) + (1 - sum_y min(p(y), q(y)))
 *   max(p(x) - q(x), 0) / sum_y max(p(y) - q(y), 0) = min(p(x), q(x)) + max(p(x) - q(x), 0) = p(x), since 1 - sum min(p, q) = sum max(p - q, 0).
 * GL3_E_ARG, before anything is enqueued: what gl3_forward_batch_verify refuses; q_slots NULL; an entry below -1 or >= max_batch on a row of
 * a sampled run that has a draft.  GL3_E_STATE: such an entry names a slot that was never written.  GL3_E_UNSUPPORTED: max_batch <= 1;
 * tp_size > 1 (this entry, gl3_verify_rows_dist and the three draft-table entries are ONE-rank, as gl3_forward_batch_verify is). */
GL3_API int32_t gl3_forward_batch_verify_dist(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions, int32_t n,
                                              const float* temperature, const float* coins, const int32_t* q_slots,
                                              gl3_verify_result* results_out, int32_t* n_runs_out);
/* Parity tap: the same decision on caller-supplied logits (host f32[n][vocab]), as gl3_verify_rows; q_slots: int32[n]. */
GL3_API int32_t gl3_verify_rows_dist(gl3_ctx* ctx, const float* logits, const int32_t* tokens, const int32_t* run_rows, int32_t n_runs,
                                     const float* temperature, const float* coins, const int32_t* q_slots, gl3_verify_result* results_out);
/* Draft chain: k single-token steps of ONE plan behind one host wait, the id each step draws fed to the next step on the device.  What a
 * draft model is called for, and plain "generate k ids without a round trip per id".
 * Equivalence: the call computes, bit for bit, what k consecutive calls gl3_forward_decode_sample(ctx, t_j, position + j, temperature, 0.f,
 * coins[j], &tokens_out[j]) compute, with t_0 = token and t_(j+1) = tokens_out[j] (topp 0: CategoricalSampler), each followed, when target
 * is not NULL, by gl3_draft_probs_put(target, slot0 + j, ctx).  After the call everything observable is what the last of those calls
 * leaves: gl3_get_sample_probs, gl3_get_x, gl3_get_buffer(0..3), the K / V rows at position .. position + k - 1, what gl3_draft_probs_put
 * would copy next, what the profiling entries take as the last (token, position), and slots slot0 .. slot0 + k - 1 of the target's table,
 * which are complete when the call returns.  temperature == 0 is a greedy chain: coins is not looked at and may be NULL.  There is no
 * top-p: a tied top-p rank is decided by the host heap, and gl3_draft_probs_put refuses a top-p row anyway.
 * The host uploads (token, position), the row's settings and the k coins once and enqueues, per step, the decode step of position + j (the
 * captured step of that position's attention regime, or launch by launch under GL3_FLAG_NO_GRAPH, exactly as gl3_forward_decode_sample
 * chooses), the sampler's launches and one hand-over launch; it waits once and 4 * k bytes come back.
 * KV contract: the K / V rows of all k positions are written.  Rows past what the caller keeps (drafts a verification rejected) are
 * overwritten by the next run from the first position not kept, as with gl3_forward_batch_verify.
 * Refusals, all before anything is uploaded or enqueued; a refused call leaves KV, the sampler state and the target's table untouched.
 * GL3_E_ARG: ctx or tokens_out NULL; k <= 0 or k > GL3_CHAIN_MAX; token outside the vocabulary; position < 0 or position + k > the context
 * length; temperature negative or NaN; temperature > 0 with coins NULL or a coin outside [0, 1); target == ctx; slot0 < 0 or slot0 + k >
 * the target's max_batch; different vocabularies; plans on different devices.  GL3_E_STATE: ctx or target before gl3_finalize; a target
 * with temperature == 0 (a greedy step has no row, which is what gl3_draft_probs_put answers).  GL3_E_UNSUPPORTED: tp_size > 1 on ctx; a
 * target gl3_draft_probs_put would refuse (no max_batch > 1, or tp_size > 1).  The chain is ONE-rank: under folded gathers the peers' step
 * counters would have to advance together, which nobody has looked at.  A step that fails midway with a HIP error returns it; the plan is
 * then in the state any failed forward leaves. */
#define GL3_CHAIN_MAX 64
GL3_API int32_t gl3_forward_decode_chain(gl3_ctx* ctx, int32_t token, int32_t position, int32_t k, float temperature,
                                         const float* coins /* f32[k] or NULL */, gl3_ctx* target /* or NULL */, int32_t slot0,
                                         int32_t* tokens_out /* int32[k] */);
/* Batched draft chain: k STATIC-BATCHED decode steps of one plan behind one host wait, every row's id fed to its next step on the device.
 * What a draft plan that serves many requests is called for: one pass over its weights per step whatever the number of requests.
 * Rows: k_i = k_rows ? k_rows[i] : k steps for row i.  k_rows must be non-increasing with k_rows[0] == k and every entry in [1, k], so the
 * rows of step j are the prefix 0 .. n_j - 1 with n_j = #{i : k_i > j}; no row is ever compacted.
 * Equivalence: the call computes, bit for bit, what these k calls compute: gl3_forward_decode_batch_sample(ctx, t_j, seq_ids,
 * positions + j, n_j, temperature, topp = 0, coins + j * n, tokens_out + j * n), with t_0 = tokens and t_(j+1)[i] = tokens_out[j][i]
 * ("positions + j": every position plus j), each followed, when target is not NULL, for every row i < n_j with slots[i] >= 0, by
 * gl3_draft_probs_put_row(target, slots[i] + j, ctx, i).  tokens_out[j][i] with i >= n_j is set to -1.  temperature[i] == 0 makes row i
 * greedy in every step: its coins are not looked at, and coins may be NULL when every row is greedy.  There is no top-p, for the reason
 * gl3_forward_decode_chain gives.
 * After the call everything observable is what the last of those calls leaves: gl3_get_sample_probs_row, gl3_get_buffer(3..6),
 * gl3_get_attn_rows, gl3_get_topp_counts (unchanged), the K / V rows at positions[i] .. positions[i] + k_i - 1 of seq_ids[i], and the
 * target's slots, which are complete when the call returns.
 * The host stages tokens, sequence ids and positions once, the rows' sampler settings with the step-0 coins once and the [k][n] coins
 * once, and enqueues, per step, the static-batched step of n_j rows (the captured step of that row count while the deepest row is in the
 * one-launch attention's range, launch by launch past it or under GL3_FLAG_NO_GRAPH, exactly as gl3_forward_decode_batch_sample
 * chooses), the batched sampler's launches unless every row of the step is greedy, and one hand-over launch; it waits once and
 * 4 * k * n bytes come back.
 * KV contract: the chain's.  The K / V rows of all k_i positions of row i are written; rows of drafts that a verification rejects are
 * overwritten by the next run from the first position not kept.
 * Refusals, all before anything is uploaded or enqueued; a refused call leaves KV, the sampler state and the target's table untouched.
 * GL3_E_ARG: ctx, tokens, seq_ids, positions, temperature or tokens_out NULL; n <= 0 or n > max_batch; k outside [1, GL3_CHAIN_MAX];
 * k_rows not non-increasing, k_rows[0] != k or an entry outside [1, k]; a token or sequence id out of range or a duplicate sequence id;
 * positions[i] < 0 or positions[i] + k_i > the context length; a temperature negative or NaN; a sampled row with coins NULL or one of its
 * k_i coins outside [0, 1); target == ctx; target with slots NULL; a slot below -1, or a slot range [slots[i], slots[i] + k_i) that
 * leaves [0, max_batch) of the target or overlaps another row's; different vocabularies; plans on different devices.  GL3_E_STATE: ctx
 * or target before gl3_finalize; a greedy row with slots[i] >= 0.  GL3_E_UNSUPPORTED: ctx without max_batch > 1; tp_size > 1 on ctx (the
 * reason of gl3_forward_decode_chain); a target gl3_draft_probs_put would refuse (no max_batch > 1, or tp_size > 1). */
GL3_API int32_t gl3_forward_decode_batch_chain(gl3_ctx* ctx, const int32_t* tokens, const int32_t* seq_ids, const int32_t* positions, int32_t n,
                                               int32_t k, const int32_t* k_rows /* int32[n] or NULL */, const float* temperature /* f32[n] */,
                                               const float* coins /* f32[k][n] or NULL */, gl3_ctx* target /* or NULL */,
                                               const int32_t* slots /* int32[n] or NULL */, int32_t* tokens_out /* int32[k][n] */);
/* Test hook, no plan and no device: the host-side plan of a mixed step (csrc/gl3_batch_plan.h) for a plan with n_seqs sequence slots,
 * context length ctx and room for `capacity` rows.  runs_out / tiles_out: int32[.][4] = {first row, rows, sequence, position of the
 * first row}, room for n records each (tiles: at most 8 rows, never across a run boundary, deepest last position first); out_rows:
 * int32[n].  GL3_E_ARG for what gl3_forward_batch refuses about (seq_ids, positions, n). */
GL3_API int32_t gl3_debug_batch_plan(const int32_t* seq_ids, const int32_t* positions, const int8_t* want_logits, int32_t n,
                                     int32_t n_seqs, int32_t ctx, int32_t capacity, int32_t* runs_out, int32_t* n_runs,
                                     int32_t* tiles_out, int32_t* n_tiles, int32_t* out_rows, int32_t* n_out);
/* Test hook, no plan and no device: that plan's attention tiles split by depth (batch_plan_split).  fused_max_pos = the largest last position
 * a tile may have in the one-launch table form (-1: every row is deep; >= ctx: shallow_out is gl3_debug_batch_plan's tiles_out and nothing
 * is deep).  shallow_out: the tiles with last position <= fused_max_pos, deepest last position first; deep_out: records of at most 16 rows
 * cut from each run's deep suffix, starting at its first deep row, never across a run boundary, deepest last position first (both
 * int32[.][4] as above, room for n records each); deep_rows: int32[n], the step rows of the deep records, ascending.  GL3_E_ARG as
 * gl3_debug_batch_plan. */
GL3_API int32_t gl3_debug_batch_plan_split(const int32_t* seq_ids, const int32_t* positions, int32_t n, int32_t n_seqs, int32_t ctx,
                                           int32_t capacity, int32_t fused_max_pos, int32_t* shallow_out, int32_t* n_shallow,
                                           int32_t* deep_out, int32_t* n_deep, int32_t* deep_rows, int32_t* n_deep_rows);
/* Test hook, no plan and no device: the attention launches of one single-token decode step (csrc/gl3_decode_attn.h: attn_regime, attn_plan)
 * for a rank with heads_l query and kv_heads_l kv heads of head_size elements (kvmul query heads per kv head), context length ctx, `window`
 * softmax positions kept in LDS, the two-launch pair below position attn_mid, at position pos.  head_kernel_allowed = 0: a plan made under
 * GL3_NO_FUSED_ATTN=1.  regime_out: 0 long, 1 short (attn_head_kernel), 2 mid.  launches_out: int64[4][6] = {kernel (0 attn_head_kernel,
 * 1 attn_scores_kernel, 2 attn_scores_loop_kernel, 3 attn_softmax_pv_kernel, 4 attn_exp_kernel, 5 attn_sum_kernel, 6 attn_pv_kernel),
 * grid x, grid y, block, dynamic LDS bytes, the kernel's LDS cap} in launch order, *n_launches of them.  head_out: int64[3] =
 * {attn_head_smem(head_size, group), whether attn_head_kernel admits the head size with one query head per workgroup, and with `group`}.
 * GL3_E_ARG for a shape gl3_create refuses on these numbers or a position outside the context. */
GL3_API int32_t gl3_debug_decode_attn_plan(int32_t head_size, int32_t kvmul, int32_t heads_l, int32_t kv_heads_l, int32_t ctx, int32_t window,
                                           int32_t attn_mid, int32_t head_kernel_allowed, int32_t pos, int32_t group, int32_t* regime_out,
                                           int64_t* launches_out, int32_t* n_launches, int64_t* head_out);
/* Test hook, no plan and no device: the choice a batched step makes for ONE GEMM of the f32-activation weight types
 * (csrc/gl3_prefill_vl.h: vl_gemm_plan, what launch_gemm_vl launches) — a matrix of `rows` rows of weight_type (GL3_TYPE_F16, GL3_TYPE_Q4_0,
 * or GL3_TYPE_Q8_0 with GL3_FLAG_F32_ACTIVATION in flags; GL3_FLAG_VECTOR_512 with F16 only) over ntok tokens (chunk tokens, batched decode
 * rows, or the output rows of the logits launch).  out: int32[7] = {kernel (0 gemm_f16_mfma_kernel, 1 gemm_f16_mfma_v512_kernel,
 * 2 gemm_vlq_kernel, 3 gemm_vlq_mfma_kernel), row tiles of 64, token tiles (64 tokens; 16 for gemm_vlq_kernel), grid, and for
 * gemm_vlq_mfma_kernel: 1 = token tiles pinned to XCDs (vqm_tile_of) / 0 = vl_tile_of, token groups G and row parts P = 8 / G of vqm_groups
 * (0, 0, 0 for the other kernels; G = P = 0 under GL3_VQM_XCD_TOKENS=0)}.  Q4_0 / Q8_0 take gemm_vlq_mfma_kernel when ntok > 16 and
 * row tiles * ceil(ntok / 64) >= 192.  The answer depends on the process's switches, read once: GL3_VLQ_MFMA=0 (never the matrix-pipe kernel),
 * GL3_VQM_XCD_TOKENS=0, and the diagnostic GL3_VLQ_MFMA_MIN_TILES=<t> (t > 0 replaces the 192; it puts small test shapes on the matrix-pipe
 * kernel).  GL3_E_ARG: a weight type / flag combination that gl3_create refuses or that batches elsewhere (GL3_FLAG_SCALAR_DOT,
 * GL3_FLAG_VECTOR_128, Q8_0 without GL3_FLAG_F32_ACTIVATION), rows < 1, ntok < 1, null out. */
GL3_API int32_t gl3_debug_vl_gemm_plan(int32_t weight_type, uint32_t flags, int32_t rows, int32_t ntok, int32_t out[7]);
/* Test hook, no plan and no device: the choice a batched Q8_0 step of MORE THAN 64 rows makes for ONE GEMM (csrc/gl3_prefill_gemm3.hip: g3_plan,
 * what g3_dispatch launches) — epi 0 store (qkv, logits), 1 residual (wo, down), 2 SwiGLU (gate + up, rows = hidden) over a matrix of `rows`
 * rows and ntok tokens (chunk tokens, or the output rows of the logits launch).  out: int32[9] = {kernel (0 pf_gemm3_kernel,
 * 1 pf_gemm3t_kernel), workgroup tile rows per matrix, tile tokens, blocks per K stage, NFR (row fragments of the tall tiling; 0 for
 * pf_gemm3_kernel), row tiles, token tiles, grid (tiles rounded up to 8; workgroup lin works on tile J = (lin & 7) * (grid / 8) + (lin >> 3),
 * row tile J / token tiles, token tile J % token tiles, and leaves when J is past the last tile), 1 when the gate + up launch can write hb
 * as the down projection's quantised operand (tall tiling, two blocks per stage, rows % 32 == 0)}.  Store / residual: 128 x 128 tiles when
 * ceil(rows / 128) * ceil(ntok / 128) >= 512, 96 x 128 when rows % 96 == 0 and 128 < ceil(rows / 96) * ceil(ntok / 128) <= 384, else
 * 64 x 128.  SwiGLU: the fewest tile-steps per SIMD between 128 x 128 (64 + 64 rows) and the tall tiling of NFR 4 .. 7, the first of equal
 * costs.  The answer depends on the process's switches, read once: GL3_PF_GEMM3_TALL=-1|4..7, GL3_PF_GEMM3_TALL_KB=1,
 * GL3_PF_GEMM3_SHAPE=1..4 (4: 64 x 64 tiles), GL3_PF_GEMM3_QOUT=0.  GL3_E_ARG: another epi, rows < 1, ntok < 1, null out (ntok <= 64 is
 * answered by the same rule although such a step runs bdw_gemm_kernel). */
GL3_API int32_t gl3_debug_gemm3_plan(int32_t epi, int32_t rows, int32_t ntok, int32_t out[9]);
/* Test hook, no plan and no device: the launch a batched Q8_0 step of AT MOST 64 rows makes for ONE GEMM (csrc/gl3_bd_gemm.h: bd_gemm_plan,
 * what launch_gemm launches as bdw_gemm_kernel) — epi as above over a matrix of `rows` rows and an inner dimension of k elements (a multiple
 * of 32) and ntok tokens (step rows, or the output rows of the logits launch); quantised_out != 0: the gate + up launch that writes hb as the
 * down projection's int8 operand (ignored for the other epilogues).  out: int32[12] = {token slots of the operand layout (32 up to 32
 * tokens, 64 up to 64; 0: more than 64 tokens, not this kernel, and every other field is 0 or -1), tiles in flight DA (8; SwiGLU 4), 1 when
 * the quantising form runs, threads per workgroup (64; quantising 128), token tiles of 16, units (16-row strips; quantising: 32-row strip
 * pairs), grid (units rounded up to 8, times token tiles), K tiles of 4 blocks, full trips of DA tiles, tiles of the partial last trip (0:
 * none; the last of them holds k / 32 % 4 blocks when that is not 0), and for workgroup `wg` of the grid its unit and its token tile
 * (unit = wg / (8 * token tiles) * 8 + wg % 8, token tile = wg / 8 % token tiles), both -1 when wg is outside the grid or the workgroup
 * exits at once (unit >= units)}.  GL3_E_ARG: another epi, rows < 1, k < 32 or not a multiple of 32, ntok < 1, null out. */
GL3_API int32_t gl3_debug_bd_gemm_plan(int32_t epi, int32_t rows, int32_t k, int32_t ntok, int32_t quantised_out, int32_t wg, int32_t out[12]);
/* Test hook, no plan and no device: the launch a single-token decode step makes for ONE projection of the f32-activation weight types
 * (csrc/gl3_veclane_kernels.h: vl_matvec_plan, what launch_matvec launches) — a matrix of `rows` rows and an inner dimension of k elements
 * of weight_type (GL3_TYPE_F16, GL3_TYPE_Q4_0, or GL3_TYPE_Q8_0 with GL3_FLAG_F32_ACTIVATION in flags; GL3_FLAG_SCALAR_DOT for the scalar
 * order of F16 / Q4_0, GL3_FLAG_VECTOR_512 with vector-order F16 only), pro 0 = RMSNorm in front of the product (qkv, gate + up, logits) /
 * 1 = none (wo, down), epi 0 store, 1 residual, 2 SwiGLU (gate + up, rows = hidden).  out: int32[12] = {kernel (0 matvec_rl_kernel,
 * 1 matvec_vl_kernel with the RMSNorm in its prologue, 2 matvec_vl_kernel, 3 matvec_vlq_kernel), 1 when rmsnorm_f32_kernel is launched in
 * front, wavefronts per workgroup, MAXW of matvec_vlq_kernel (8 or 16; 0 for the other kernels), grid, threads per workgroup, dynamic LDS
 * bytes, the LDS bytes the kernel may ask for, and for matvec_vlq_kernel (0 otherwise): chunks of K (256 elements of Q4_0, 128 of Q8_0),
 * rounds, chunks per wavefront and round rc, and the most a wavefront's registers hold (vq_round_chunks)}.  Scalar order: 64 rows per
 * workgroup of 9 wavefronts.  Vector order: the prologue form for pro 0, epi != 1 and 1024 <= k <= 5120 — for Q4_0 / Q8_0 only when
 * ceil(rows / 8) * (2 for SwiGLU) > 512; else F16 takes matvec_vl_kernel (2 groups of 8 rows per workgroup) and Q4_0 / Q8_0
 * matvec_vlq_kernel, one 8-row group per workgroup of 16 wavefronts below 256 groups, 8 below 512, 4 from there (8 when K has more than
 * 4 * vq_round_chunks chunks), halved down to 4 while there are fewer chunks than wavefronts.  GL3_E_ARG: a weight type / flag
 * combination gl3_create refuses or that runs matvec_q8t_kernel (Q8_0 without GL3_FLAG_F32_ACTIVATION), GL3_FLAG_VECTOR_128, another pro
 * or epi, rows < 1, a k the type does not accept (multiples of 64 for F16 and the scalar order, 256 for vector-order Q4_0, 128 for Q8_0;
 * at most 16384 in the vector order), null out. */
GL3_API int32_t gl3_debug_matvec_plan(int32_t weight_type, uint32_t flags, int32_t pro, int32_t epi, int32_t rows, int32_t k, int32_t out[12]);
/* Fork a prefix: copy the K and V rows at positions [p0, p1) of sequence src_seq, every layer, into the same positions of each of the
 * n_dst sequences dst_seqs[].  Rows outside [p0, p1) of the destinations, every other sequence and the source are untouched.
 * What the rows mean: a row's arithmetic does not depend on which rows share its step, so the K / V rows at positions 0 .. p of a sequence are
 * a function of its tokens 0 .. p alone.  After a call with p0 == 0 a destination therefore behaves, for the rows at positions >= p1 that are
 * forwarded on it next, exactly (bit for bit) as if tokens 0 .. p1 - 1 of the source had been forwarded on it.  K is stored after RoPE, so rows
 * go to the SAME positions only; there is no shifting.
 * One launch on the plan's stream, behind whatever step was enqueued last; the call returns after the copy has completed, so gl3_get_kv_seq and
 * the next step both see it.  Rank-local: under tensor parallelism a rank copies its own kv_dim / tp_size slice, and the caller invokes it on
 * every rank.  Needs n_seqs > 1, not max_batch > 1.  GL3_E_ARG, before anything is enqueued: null ctx or dst_seqs, n_dst <= 0, src_seq or a
 * destination outside [0, n_seqs), a destination equal to src_seq or listed twice, p0 < 0, p1 > ctx, p0 > p1.  p0 == p1 is a valid no-op
 * (GL3_OK, no launch).  GL3_E_STATE: before gl3_finalize. */
GL3_API int32_t gl3_kv_seq_copy(gl3_ctx* ctx, int32_t src_seq, const int32_t* dst_seqs, int32_t n_dst, int32_t p0, int32_t p1);
/* Dispatch tap: the rows of the last batched step (gl3_forward_prefill_seq, gl3_forward_decode_batch, gl3_forward_batch and their sampled
 * forms) by the attention form that served them in the last layer — out[0] attn_head_kernel (RoPE + attention in one launch per row),
 * out[1] the one-launch tiled kernels, out[2] the long-context trio (scores, softmax rows, weighted V sum), out[3] the per-row pair.  The
 * four sum to the step's n.  Host bookkeeping only.  GL3_E_STATE before any batched step, GL3_E_UNSUPPORTED without max_batch > 1. */
GL3_API int32_t gl3_get_attn_rows(gl3_ctx* ctx, int32_t out[4]);

/* Parity tap: the probabilities (f32[vocab]) row `row` of the last batched sampled step (or gl3_sample_rows call) was drawn from
 * (GL3_E_STATE for a greedy row or before any such step). */
GL3_API int32_t gl3_get_sample_probs_row(gl3_ctx* ctx, int32_t row, float* out);
/* Parity tap: the batched sampler alone on caller-supplied logits (host f32[n][vocab]); no forward pass, no KV change.  Needs a
 * plan with max_batch > 1; n <= max_batch (tp_size > 1: n <= 64, rank-chunked on the device, no peer needed: see gl3_score_rows).  The
 * logits buffer of the batched step is overwritten. */
GL3_API int32_t gl3_sample_rows(gl3_ctx* ctx, const float* logits, int32_t n, const float* temperature, const float* topp,
                                const float* coins, int32_t* tokens_out);

/* Parity taps. */
GL3_API int32_t gl3_get_x(gl3_ctx* ctx, float* out /* f32[dim] */);
GL3_API int32_t gl3_get_layer_x(gl3_ctx* ctx, int32_t layer, float* out /* f32[dim], needs GL3_FLAG_LAYER_TAPS */);
GL3_API int32_t gl3_get_kv(gl3_ctx* ctx, int32_t layer, int32_t position, float* k_out, float* v_out /* f32[kvDim/tp] */);
GL3_API int32_t gl3_get_kv_seq(gl3_ctx* ctx, int32_t seq, int32_t layer, int32_t position, float* k_out, float* v_out);

/* Debug/parity tap: copy a scratch buffer of the LAST executed layer to the host.
 * which: 0 = raw q|k|v of the qkv projection, 1 = attention output xb, 2 = hb (SwiGLU output), 3 = logits; 4 / 5 / 6 = X / AO / HB
 * of the last batched step; Qwen2-MoE routing of the last layer: 7 = weights [topk + 1] and 8 = expert ids (as floats) [topk] of
 * the last decode step, 9 = weights [rows][topk + 1] and 10 = expert ids [rows][topk] of the last batched step (rows in step order). */
GL3_API int32_t gl3_get_buffer(gl3_ctx* ctx, int32_t which, float* out, uint64_t n_floats);

/* Test hook: the strictly sequential f32 sum of squares of x[0..n) (InferenceCore.rmsnorm's reduce), evaluated
 * by the same exact parallel device routine the kernels use (1024 <= n <= 5120, multiple of 4; device = ordinal). */
GL3_API int32_t gl3_debug_sumsq(int32_t device, const float* x, int32_t n, float* out);

GL3_API int32_t gl3_reset_kv(gl3_ctx* ctx);

/* One decode step launched kernel by kernel with HIP events around every launch. */
GL3_API int32_t gl3_profile_decode(gl3_ctx* ctx, int32_t token, int32_t position, gl3_kernel_times* out);

/* Average device time of ONE kernel class, measured with a single HIP event pair around `iters` sweeps over all
 * layers (back-to-back launches of that kernel on every layer's own weights, so nothing is cache-resident).
 * klass: GL3_K_MATVEC_*; out_us = mean per launch (includes the ~1.5 us inter-kernel boundary). */
GL3_API int32_t gl3_profile_kernel(gl3_ctx* ctx, int32_t klass, int32_t iters, double* out_us, uint64_t* bytes_per_launch);

/* The batched-prefill GEMM of one class (GL3_K_MATVEC_QKV / WO / GATEUP / DOWN) at n_tokens <= max_batch tokens: mean device
 * time per launch over `iters` sweeps of all layers, and the int8 multiply-add work of one launch (2 * rows * K * n_tokens
 * operations; the activations are whatever the last prefill left in the plan's buffers — timing only, the residual stream
 * is clobbered). */
GL3_API int32_t gl3_profile_prefill_kernel(gl3_ctx* ctx, int32_t klass, int32_t n_tokens, int32_t iters, double* out_us,
                                           uint64_t* int8_ops_per_launch);

/* Measured-achievable peaks of THIS device, for the roofline denominators beside the spec-sheet figures: a streaming
 * read of 1 GiB (float4 non-temporal loads, every CU busy; three regions read in rotation so that nothing is still in the Infinity Cache), a device-to-device copy of the same size (bytes counted = read + written) and
 * a loop of independent v_mfma_i32_32x32x32_i8 on every SIMD (4 accumulators per wavefront).  Best of 3 timed repetitions each,
 * HIP events on a private stream; any out pointer may be NULL.  Needs no plan. */
GL3_API int32_t gl3_probe_peaks(int32_t device, double* hbm_read_gbs, double* hbm_copy_gbs, double* int8_mfma_tops);

/* RunMetrics slots (TornadoVMMasterPlanSingleToken.java:40-54): plan creation and weight copy-in, ms. */
GL3_API int32_t gl3_get_init_ms(gl3_ctx* ctx, double* plan_ms, double* copy_in_ms);

GL3_API void gl3_destroy(gl3_ctx* ctx);
GL3_API const char* gl3_last_error(gl3_ctx* ctx);  /* ctx may be NULL: last create error */

/* ---- native GGUF loader.  Replaces, for this path, J/tensor/GGUF.java:43-137,217-311 (header,
 * metadata, tensor infos, alignment), the config extraction of LlamaModelLoader.java:47-69 / Qwen3ModelLoader.java:48-79, the
 * tensor-name map :83-98 and RoPE.precomputeFreqsCis (J/inference/operation/RoPE.java:6-37).  The file is mmap'd; tensor
 * bytes go from the mapping straight to gl3_upload_tensor (no 2 GiB limit, no TornadoVM 16-byte header remapping). */
typedef struct gl3_gguf gl3_gguf;
GL3_API int32_t gl3_gguf_open(const char* path, gl3_gguf** out);            /* GGUF v2 / v3 */
GL3_API void gl3_gguf_close(gl3_gguf* g);
GL3_API const char* gl3_gguf_last_error(const gl3_gguf* g);                 /* g may be NULL: last open / load error */
GL3_API int32_t gl3_gguf_tensor_count(const gl3_gguf* g);
/* ne[4]: GGUF dimension order (ne[0] = row length); data points into the mapping (valid until gl3_gguf_close). */
GL3_API int32_t gl3_gguf_tensor_info(const gl3_gguf* g, int32_t i, const char** name, int32_t* type, uint64_t* ne, const void** data,
                                     uint64_t* bytes);
GL3_API int32_t gl3_gguf_meta_number(const gl3_gguf* g, const char* key, double* out);   /* any scalar numeric / bool key */
GL3_API int32_t gl3_gguf_meta_string(const gl3_gguf* g, const char* key, const char** out);
/* Shape fields of desc (arch, dim, hidden, layers, heads, head_size, vocab, rms_eps, weight_type) from the metadata; desc->ctx is
 * kept if it is > 0 and not larger than <arch>.context_length, desc->ctx = 0 selects min(context_length, 4096) (the reference
 * always clamps with Configuration.withContextLength(maxTokens)); the other fields are left as the caller set them. */
GL3_API int32_t gl3_gguf_model_desc(gl3_gguf* g, gl3_model_desc* desc, float* rope_theta);
/* RoPE.precomputeFreqsCis with ropeScaling = false: cr / ci are f32[ctx * head_size/2]. */
GL3_API void gl3_rope_table(int32_t ctx, int32_t head_size, float theta, float* cr, float* ci);
/* RoPE.precomputeFreqsCisYaRN (J/inference/operation/RoPE.java:39-83; Devstral 2, DevstralModelLoader.java:76-110): ramp between the
 * plain and the / factor frequency per pair, cos / sin scaled by mscale = 1 + 0.1 * log_multiplier * ln(factor) (1 when
 * log_multiplier <= 0).  gl3_load_gguf builds this table when <arch>.rope.scaling.type == "yarn". */
GL3_API void gl3_rope_table_yarn(int32_t ctx, int32_t head_size, float theta, float factor, float beta_fast, float beta_slow,
                                 float log_multiplier, int32_t original_ctx, float* cr, float* ci);
/* <arch>.rope.scaling.{factor, yarn_beta_fast, yarn_beta_slow, yarn_log_multiplier (default 0), original_context_length}
 * (DevstralModelLoader.java:80-86): returns 1 and fills them for a "yarn" file, 0 for a file with the plain table. */
GL3_API int32_t gl3_gguf_yarn_params(gl3_gguf* g, float* factor, float* beta_fast, float* beta_slow, float* log_multiplier,
                                     int32_t* original_ctx);
/* ModelLoader.dequantizeToQ8_0TornadoTensor (J/model/loader/ModelLoader.java:173-224): the load-time conversion the reference's GPU
 * path applies to Q4_K / Q5_K / Q6_K tensors — element-wise getFloat of the CPU tensor classes (Q4_KFloatTensor.java:86-114,
 * Q5_KFloatTensor.java:86-120, Q6_KFloatTensor.java) re-quantised to Q8_0 blocks.  n_elements % 256 == 0; dst: n / 32 * 34 bytes.
 * gl3_load_gguf applies it to every K-quant tensor; a host that uploads tensors itself can call it first. */
GL3_API int32_t gl3_kquant_to_q8_0(int32_t src_type, const void* src, uint64_t n_elements, void* dst);

/* open + gl3_create + one gl3_upload_tensor per tensor + RoPE table + gl3_finalize (not finalized when opts->tp_size > 1 or
 * GL3_FLAG_FORCE_RCCL is set: call gl3_tp_init / gl3_tp_attach_local and gl3_finalize).  opts may be NULL; it supplies
 * ctx / max_batch / device / tp_rank / tp_size / flags / n_seqs. */
GL3_API int32_t gl3_load_gguf(const char* path, const gl3_model_desc* opts, gl3_ctx** out);

#ifdef __cplusplus
}
#endif
#endif
