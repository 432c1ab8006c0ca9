"""The inner-dimension grid: the K (dim, or hidden for the down projection) at which a projection kernel changes form or a plan is refused,
per weight type, and the rule that says which form a K runs.

Every case is a Llama model of 2 layers, 8 query heads on 2 kv heads of 32 elements (q_dim 256: a multiple of 64, 128 and 256, so every
weight type accepts it whatever dim is), hidden 256, vocab 96, ctx 96; only dim varies (head_size * n_heads need not be dim).  The hidden
cases swap the roles: dim 256, hidden varies.  The MoE cases are tiny-qwen2moe (8 experts, top-2, experts of 128) with dim overridden.
Two vector-order cases of the K-split types carry a vocabulary of 4112 rows: 514 8-row groups, more than the 512 below which the logits
launch of such a type keeps the separate RMSNorm launch at every K (launch_matvec, gl3_api.hip).

The rule below restates, in Python, conditions of gl3_decode_kernels.h (matvec_q8t_kernel), gl3_prefill.hip (pf_norm_quant_kernel, nq_smem),
gl3_rowlane_kernels.h (rmsnorm_f32_kernel), gl3_veclane_kernels.h (vl_rms_fusable, vl_smem_bytes), gl3_moe_kernels.h (moe_router_token,
moe_router_smem) and gl3_api.hip (matvec_smem, launch_matvec, gl3_create).  tests/test_k_shapes.py asserts what the grid covers, that every
row is needed for it and that the limits equal the library's; tests/test_gpu_k_shapes.py runs the grid."""

SS_LO, SS_HI = 1024, 5120          # exact_sumsq_lds serves SS_LO <= K <= SS_HI, seq_sum_lds on one wavefront everything else
Q8_RMS_QUADS, Q8_QUANT_QUADS = 5, 14      # matvec_q8t_kernel: activation quads per aux thread held in registers (NXV), RMS / plain prologue
MOE_QJ = 2                         # moe_router_token: quads per thread and row loaded ahead of the sum of squares
MOE_RR = 8                         # router rows per workgroup
LDS_MAX = 160 * 1024 - 256         # hipFuncAttributeMaxDynamicSharedMemorySize of every large-LDS kernel
VL_LDS_MAX = 64 * 1024             # the vector-order matvecs stay under the dynamic default
RL_LDS_MAX = 150 * 1024            # gl3_create: rl_smem_bytes(max(dim, hidden), EPI_STORE)
KSPLIT_MIN_WAVES = 513             # launch_matvec: a K-split type fuses the RMSNorm prologue only with more than 512 8-row groups

#         kind       weight type, plan flags, oracle (vector_bits, f32_activation), legal step of dim, batched path
KINDS = {
    "q8":      dict(wtype=8, flags=(), oracle=(0, False), step=32, batched=True),
    "q8h":     dict(wtype=8, flags=(), oracle=(0, False), step=32, batched=True),                      # dim 256, the K is hidden
    "f16v256": dict(wtype=1, flags=(), oracle=(256, False), step=64, batched=True),
    "f16v512": dict(wtype=1, flags=("FLAG_VECTOR_512",), oracle=(512, False), step=64, batched=True),
    "q4v256":  dict(wtype=2, flags=(), oracle=(256, False), step=256, batched=True),
    "f16s":    dict(wtype=1, flags=("FLAG_SCALAR_DOT",), oracle=(0, False), step=64, batched=False),   # prefill is token by token
    "q4s":     dict(wtype=2, flags=("FLAG_SCALAR_DOT",), oracle=(0, False), step=64, batched=False),
    "q8f32":   dict(wtype=8, flags=("FLAG_F32_ACTIVATION",), oracle=(256, True), step=128, batched=True),
    "moe":     dict(wtype=8, flags=(), oracle=(0, False), step=32, batched=True),
}
N_EXPERTS = 8
BIG_VOCAB = 4112                   # 514 8-row groups; a multiple of 16
HEADS, KV_HEADS, HEAD_SIZE, HIDDEN, VOCAB, CTX, LAYERS = 8, 2, 32, 256, 96, 96, 2


# ---- the rule
def ss_scratch_bytes(n):
    return 128 + 3 * n


def sumsq_form(k):
    """Which sum of squares an RMSNorm over k elements runs, in all five copies of the split"""
    return "exact" if SS_LO <= k <= SS_HI and k % 4 == 0 else "seq"


def q8_rms_in_registers(k):
    """matvec_q8t_kernel<PRO_RMS>: the row stays in registers between the sum of squares and the quantiser (else re-read from memory)"""
    return k // 4 <= Q8_RMS_QUADS * 256


def q8_quant_in_registers(k):
    """matvec_q8t_kernel<PRO_QUANT> (wo, down)"""
    return k // 4 <= Q8_QUANT_QUADS * 256


def vl_fuse_rms(k, rows, ksplit_type, swiglu=False, resid=False):
    """launch_matvec, vector order: the RMSNorm runs in matvec_vl_kernel's prologue (else rmsnorm_f32_kernel in front of the matvec)"""
    waves = (rows + 7) // 8 * (2 if swiglu else 1)
    return sumsq_form(k) == "exact" and not resid and not (ksplit_type and waves < KSPLIT_MIN_WAVES)


def moe_router_in_registers(dim):
    return dim // 4 <= MOE_QJ * 256


def nq_smem(k):
    """pf_norm_quant_kernel<PQ_NORM | PQ_NORM_F32>, and the same bytes for rmsnorm_f32_kernel"""
    return (k + 32) * 4 + ss_scratch_bytes(k) + 64


rmsnorm_smem = nq_smem


def matvec_smem(pro, epi, k):
    """matvec_q8t_kernel.  pro: "rms" | "quant"; epi: "store" | "resid" | "swiglu" """
    ng, nm = (k // 32 + 3) // 4, 2 if epi == "swiglu" else 1
    return ng * 4 * 32 + ng * 4 * 4 + ((k + 32) * 4 if pro == "rms" else 0) + 2 * nm * ng * 64 * 4 + 128


def moe_router_smem(dim, experts):
    return (dim + 32) * 4 + ss_scratch_bytes(dim) + ((experts + 7) & ~3) * 4 + 64 + MOE_RR * (dim + 4) * 4


def vl_smem_bytes(k):
    return k * 4


def rl_smem_bytes(k, swiglu=False):
    return (k + 2 * (2 if swiglu else 1) * 64 * 68) * 4


def largest(fits, step):
    """the largest multiple of `step` for which fits() holds (fits is monotone)"""
    k = step
    while fits(k + step):
        k += step
    return k


def q8_dim_fits(dim, batched=True):
    return (matvec_smem("rms", "store", dim) <= LDS_MAX and matvec_smem("rms", "swiglu", dim) <= LDS_MAX and
            (not batched or nq_smem(dim) <= LDS_MAX))


Q8_MAX_DIM = largest(q8_dim_fits, 32)                                                       # 12416: the gate/up launch
Q8_MAX_HIDDEN = largest(lambda k: matvec_smem("quant", "resid", k) <= LDS_MAX, 32)          # 31872: the down launch
NQ_MAX_K = largest(lambda k: nq_smem(k) <= LDS_MAX, 32)                                     # 23296: never the binding limit of a Q8_0 plan
VL_MAX_K = largest(lambda k: vl_smem_bytes(k) <= VL_LDS_MAX, 64)                            # 16384
SCALAR_MAX_DIM = largest(lambda k: rmsnorm_smem(k) <= LDS_MAX and rl_smem_bytes(k) <= RL_LDS_MAX and rl_smem_bytes(k, True) <= LDS_MAX, 64)   # 23296
MOE_MAX_DIM = largest(lambda k: moe_router_smem(k, N_EXPERTS) <= LDS_MAX and q8_dim_fits(k), 32)   # 4160: the router

#  name -> (kind, the K of the case, vocab)
GRID = {}


def _rows(kind, ks, vocab=VOCAB):
    for k in ks:
        GRID["%s-%d" % (kind, k)] = (kind, k, vocab)


_rows("q8", [992, 1024, 5120, 5152, 8192, Q8_MAX_DIM])
_rows("q8h", [14336, 14368, 18944, Q8_MAX_HIDDEN])
_rows("f16v256", [960, 1024, 5120, 5184, 8192, VL_MAX_K])
_rows("f16v512", [5120, 5184])
_rows("q4v256", [768, 1024])
_rows("q4v256", [5120, 5376], BIG_VOCAB)
_rows("f16s", [960, 1024, 5120, 5184, SCALAR_MAX_DIM])
_rows("q4s", [960, 1024, 5120, 5184])
_rows("q8f32", [896, 1024])
_rows("q8f32", [5120, 5248], BIG_VOCAB)
_rows("moe", [992, 1024, 2048, 2080, 3584, MOE_MAX_DIM])

# the next legal step above a limit: gl3_create answers GL3_E_UNSUPPORTED.  (kind, field, value, what the message names)
REFUSED = [("q8", "dim", Q8_MAX_DIM + 32, "dim = %d" % (Q8_MAX_DIM + 32)),
           ("q8h", "hidden", Q8_MAX_HIDDEN + 32, "hidden = %d" % (Q8_MAX_HIDDEN + 32)),
           ("f16s", "dim", SCALAR_MAX_DIM + 64, "dim = %d" % (SCALAR_MAX_DIM + 64)),
           ("f16v256", "dim", VL_MAX_K + 64, "16384"),
           ("moe", "dim", MOE_MAX_DIM + 32, "dim")]


def dims_of(name):
    """(dim, hidden) of a case"""
    kind, k, _ = GRID[name]
    return (256, k) if kind == "q8h" else (k, HIDDEN)


def case_config(synth, name):
    kind, k, vocab = GRID[name]
    dim, hidden = dims_of(name)
    if kind == "moe":
        b = synth.CONFIGS["tiny-qwen2moe"]
        assert (b.n_experts, b.n_experts_used, b.moe_hidden, b.n_heads * b.head_size) == (N_EXPERTS, 2, 128, 256)
        return synth.ModelConfig(**{**b.__dict__, "name": "k-" + name, "dim": dim, "hidden": hidden, "vocab": vocab, "ctx": CTX})
    return synth.ModelConfig("k-" + name, synth.ARCH_LLAMA, dim, hidden, LAYERS, HEADS, KV_HEADS, HEAD_SIZE, vocab, CTX, 1e-5, 500000.0, False)


def case_model(pkg, name, seed=41):
    return pkg.synth.make_numpy(case_config(pkg.synth, name), wtype=KINDS[GRID[name][0]]["wtype"], seed=seed)


def case_flags(hip, name):
    f = 0
    for n in KINDS[GRID[name][0]]["flags"]:
        f |= getattr(hip, n)
    return f


# ---- which of the five copies of the sum-of-squares split a case runs, and in which form
def sumsq_copies(name):
    """{(copy, form)} over the launches of the case: copy in "q8t" (matvec_q8t_kernel), "pf" / "pf_f32" (pf_norm_quant_kernel<PQ_NORM> /
    <PQ_NORM_F32>), "rmsnorm" (rmsnorm_f32_kernel), "vl" / "vl_ksplit" (the fused prologue of matvec_vl_kernel), "router"."""
    kind, _, vocab = GRID[name]
    dim, hidden = dims_of(name)
    form, out = sumsq_form(dim), set()
    if kind in ("q8", "q8h", "moe"):
        out |= {("q8t", form), ("pf", form)}
        if kind == "moe":
            out.add(("router", form))
    elif kind in ("f16s", "q4s"):
        out.add(("rmsnorm", form))
    else:
        ksplit = kind in ("q4v256", "q8f32")
        out.add(("pf_f32", form))
        for rows, swiglu in ((HEADS * HEAD_SIZE + 2 * KV_HEADS * HEAD_SIZE, False), (hidden, True), (vocab, False)):      # qkv, gate/up, logits
            if vl_fuse_rms(dim, rows, ksplit, swiglu):
                out.add(("vl_ksplit" if ksplit else "vl", form))
            else:
                out.add(("rmsnorm", form))
    return out


def position(kind, k):
    """where a K sits against the two boundaries of the split, by the kind's legal step"""
    step = KINDS[kind]["step"]
    below = (SS_LO - 1) // step * step
    return {below: "last below 1024", SS_LO: "1024", SS_HI: "5120", (SS_HI // step + 1) * step: "first above 5120"}.get(k)


# per kind: the positions, and the named dims beyond them, that the grid must hold
WANTED = {
    "q8": ["last below 1024", "1024", "5120", "first above 5120", 8192, Q8_MAX_DIM],
    "f16v256": ["last below 1024", "1024", "5120", "first above 5120", 8192, VL_MAX_K],
    "f16v512": ["5120", "first above 5120"],
    "q4v256": ["last below 1024", "1024", "5120", "first above 5120"],
    "f16s": ["last below 1024", "1024", "5120", "first above 5120", SCALAR_MAX_DIM],
    "q4s": ["last below 1024", "1024", "5120", "first above 5120"],
    "q8f32": ["last below 1024", "1024", "5120", "first above 5120"],
    "q8h": [Q8_QUANT_QUADS * 1024, Q8_QUANT_QUADS * 1024 + 32, 18944, Q8_MAX_HIDDEN],      # both sides of the plain prologue's register split, Qwen2.5-7B
    "moe": ["last below 1024", "1024", MOE_QJ * 1024, MOE_QJ * 1024 + 32, 3584, MOE_MAX_DIM],   # ... of the router's, Qwen2-57B-A14B
}


def missing(names):
    """Requirements that the cases `names` do not meet (empty: the grid covers everything)"""
    have = set()
    for n in names:
        kind, k, _ = GRID[n]
        have.add((kind, k))
        if position(kind, k):
            have.add((kind, position(kind, k)))
    req = [("%s: %s" % (kind, w), (kind, w) in have) for kind, ws in WANTED.items() for w in ws]
    copies = set().union(*[sumsq_copies(n) for n in names]) if names else set()
    for copy in ("q8t", "pf", "pf_f32", "rmsnorm"):
        for form in ("exact", "seq"):
            req.append(("sum of squares of %s, %s form" % (copy, form), (copy, form) in copies))
    for copy in ("vl", "vl_ksplit", "router"):          # the fused prologue exists in the exact range only; the router's dim ends below 5120
        req.append(("sum of squares of %s, exact form" % copy, (copy, "exact") in copies))
    req.append(("sum of squares of router, seq form", ("router", "seq") in copies))
    return [what for what, ok in req if not ok]
