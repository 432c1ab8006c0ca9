"""The attention shape grid: head sizes and kvMul (query heads per kv head) that gl3_create accepts and no synth config has, and the dispatch
rule that says which decode / batched attention kernels such a shape runs at a depth.

Every shape is a tiny config (dim 256, hidden 512, 2 layers, vocab 512) with head_size, n_heads, n_kv_heads and ctx overridden; the base
config names the family: tiny-llama (adjacent-pair RoPE), tiny-qwen3 (per-head q / k RMSNorm, NeoX RoPE), tiny-qwen2 (q / k / v bias),
tiny-phi3 (fused qkv tensor, NeoX RoPE), tiny-granite (attention scale instead of 1 / sqrt(head size)).  head_size * n_heads need not
be dim.  tests/test_attn_shapes.py asserts what the grid covers (and that every row is needed for it), tests/test_gpu_attn_shapes.py runs it.

The dispatch rule below restates in Python the decode attention plan of csrc/gl3_decode_attn.h (attn_regime, attn_plan, the LDS sizes beside
the kernels and their caps) and the conditions of gl3_prefill.hip (pf_fused_decode, pf_attention); the GPU tests compute what
plan.attn_rows() must report from it.  tests/test_attn_shapes.py holds the decode part equal to the library's own plan, asked through
gl3_debug_decode_attn_plan, over every head size, kvMul, regime boundary and switch."""

AF_MAXN = 128          # gl3_decode_attn.h: positions below it take attn_head_kernel where the shape admits it
ATTN_MID = 768         # gl3_decode_attn.h (ATTN_MID_DEFAULT; GL3_ATTN_MID): positions below it (and >= AF_MAXN, or from 0 without attn_head_kernel) take the two-launch pair
PV_ROWS = 1024         # V rows of one slab of attn_softmax_pv_kernel
PV_G = 4               # query heads per head quad of attn_pv_kernel
LDS_MAX = 150 * 1024   # what attn_head_kernel may ask for (ATTN_HEAD_LDS_CAP: gl3_create's fused_attn_ok and pf_attention's bd_group)

# the single-token decode walk of tests/test_gpu_attn_shapes.py: a context that is a multiple of 4 (pf_softmax_rows_kernel) past PV_ROWS and 16 score
# tiles; decode steps at the start, across AF_MAXN, across ATTN_MID and past PV_ROWS, batched prefill between them; prompt rows compared on both
# sides of 64, 128, 768 and 1024 (125 / 131 and 765 / 770: the nearest rows that no decode step wrote)
CTX = 1100
DECODE_AT = [0, 1, 2, 3, 126, 127, 128, 129, 130, 766, 767, 768, 769, 1030, 1031]
PREFILL_KV_AT = [63, 64, 125, 131, 765, 770, 1023, 1024]

#        name                 base config     head size  heads  kv heads
SHAPES = {
    # head sizes without attn_head_kernel and without tiled prefill kernels, one family each
    "qwen3-hs256-kv2":    ("tiny-qwen3",   256, 4, 2),      # qk-norm over 256 elements on 64 lanes
    "qwen3-hs160-kv5":    ("tiny-qwen3",   160, 10, 2),     # qk-norm, not a power of two; ragged head quad 4 + 1
    "qwen2-hs192-kv3":    ("tiny-qwen2",   192, 6, 2),      # q / k / v bias
    "phi3-hs224-kv1":     ("tiny-phi3",    224, 4, 4),      # fused qkv rows, multi-head attention
    "granite-hs160-kv2":  ("tiny-granite", 160, 4, 2),      # attention scale
    "llama-hs256-kv16":   ("tiny-llama",   256, 16, 1),     # the largest LDS request of the scores kernels; the one shape with a single kv head
    # kvMul 2 and 3 at head sizes 64 and 128: attn_scores_loop_kernel<64 | 128> with 2 or 3 chain wavefronts from position 768
    "llama-hs64-kv2":     ("tiny-llama",   64, 8, 4),
    "qwen3-hs64-kv3":     ("tiny-qwen3",   64, 6, 2),
    "qwen2-hs128-kv2":    ("tiny-qwen2",   128, 4, 2),
    "llama-hs128-kv3":    ("tiny-llama",   128, 6, 2),
    # kvMul 5 - 16: attn_scores_kernel with 64 x kvMul threads at every depth, ragged head quads in attn_exp / attn_sum / attn_pv_kernel
    "llama-hs64-kv5":     ("tiny-llama",   64, 10, 2),      # quads 4 + 1
    "qwen3-hs128-kv7":    ("tiny-qwen3",   128, 14, 2),     # quads 4 + 3
    "llama-hs64-kv8":     ("tiny-llama",   64, 16, 2),      # quads 4 + 4
    "llama-hs128-kv16":   ("tiny-llama",   128, 32, 2),     # four quads; static-batched decode: one query head per workgroup
    "llama-hs32-kv16":    ("tiny-llama",   32, 32, 2),      # workgroups of 1024 threads on 32-element heads
}
FAMILY = {"tiny-llama": "llama", "tiny-qwen3": "qwen3", "tiny-qwen2": "qwen2", "tiny-phi3": "phi3", "tiny-granite": "granite"}


def kvmul_of(name):
    _, _, heads, kv_heads = SHAPES[name]
    return heads // kv_heads


def head_size_of(name):
    return SHAPES[name][1]


def shape_config(synth, name, ctx):
    base, hs, heads, kv_heads = SHAPES[name]
    b = synth.CONFIGS[base]
    assert (b.dim, b.hidden, b.n_layers, b.vocab) == (256, 512, 2, 512), base
    return synth.ModelConfig(**{**b.__dict__, "head_size": hs, "n_heads": heads, "n_kv_heads": kv_heads, "ctx": ctx})


def shape_model(pkg, name, ctx, seed, wtype=8):
    return pkg.synth.make_numpy(shape_config(pkg.synth, name, ctx), wtype=wtype, seed=seed)


# ---- the dispatch rule
def attn_head_smem(hs, group=1):
    """bytes of LDS of attn_head_kernel: q[group][hs] | K[128][hs + 4] | V[128][hs] | e[group][128] | rope row | red[16]"""
    return (group * hs + AF_MAXN * (hs + 4) + AF_MAXN * hs + group * AF_MAXN + hs + 16) * 4


def has_head_kernel(hs):
    """gl3_create: fused_attn_ok (without GL3_NO_FUSED_ATTN)"""
    return attn_head_smem(hs) <= LDS_MAX


def scores_kernel_lds(hs, kvmul):
    """bytes of dynamic LDS of attn_scores_kernel: q[kvMul][hs] | K[64][hs + 4] | rope row"""
    return (kvmul * hs + 64 * (hs + 4) + hs) * 4


def decode_regime(hs, kvmul, pos, head_kernel=True, attn_mid=ATTN_MID):
    """The kernels of a single-token decode step at `pos` (attn_plan); head_kernel=False: a plan made under GL3_NO_FUSED_ATTN=1; attn_mid: GL3_ATTN_MID.
    "head": attn_head_kernel.  "pair": attn_scores_kernel + attn_softmax_pv_kernel.  "long-loop" / "long-tile": attn_scores_loop_kernel /
    attn_scores_kernel, then attn_exp_kernel, attn_sum_kernel, attn_pv_kernel."""
    if head_kernel and has_head_kernel(hs) and pos < AF_MAXN:
        return "head"
    if pos < attn_mid:
        return "pair"
    return "long-loop" if kvmul <= 4 and hs in (64, 128) else "long-tile"


def bd_group(hs, kvmul):
    """query heads per workgroup of attn_head_kernel in a static-batched step (pf_attention): the kv head's whole group while it fits"""
    return kvmul if kvmul <= 8 and attn_head_smem(hs, kvmul) <= LDS_MAX else 1


def batched_rows(hs, positions):
    """plan.attn_rows() of a static-batched decode step with rows at `positions`: [attn_head_kernel, one-launch tiled, trio, per-row pair]"""
    n = len(positions)
    return [n, 0, 0, 0] if has_head_kernel(hs) and max(positions) < AF_MAXN else [0, 0, 0, n]


def has_tiled_prefill(hs, kvmul):
    """pf_tiled_shape at a context that is a multiple of 4 and >= 64, no switches: the shapes whose prompt rows leave the per-row pair"""
    return kvmul <= 16 and hs in (32, 64, 96, 128)


# ---- what the grid has to cover; every entry: (requirement, predicate over the set of shape names)
def _shapes(names, pred):
    return [n for n in names if pred(FAMILY[SHAPES[n][0]], SHAPES[n][1], kvmul_of(n), SHAPES[n][3])]


def missing(names):
    """Requirements that the shapes `names` do not meet (empty: the grid covers everything)"""
    has = lambda pred: bool(_shapes(names, pred))
    req = []
    for hs in (160, 192, 224, 256):
        req.append(("head size %d" % hs, has(lambda f, h, m, kv: h == hs)))
    req.append(("head size 256 at kvMul 16", has(lambda f, h, m, kv: (h, m) == (256, 16))))
    for m_ in (2, 3):
        for hs in (64, 128):
            req.append(("loop scores kernel: kvMul %d at head size %d" % (m_, hs), has(lambda f, h, m, kv: (h, m) == (hs, m_))))
    for m_ in (5, 7, 8, 16):
        req.append(("tile scores kernel: kvMul %d at head size 64 or 128" % m_, has(lambda f, h, m, kv: m == m_ and h in (64, 128))))
    req.append(("1024-thread workgroups: kvMul 16 at head size 32", has(lambda f, h, m, kv: (h, m) == (32, 16))))
    for m_ in (5, 7, 8):
        req.append(("attn_head_kernel group form G = %d" % m_, has(lambda f, h, m, kv: m == m_ and has_head_kernel(h) and bd_group(h, m) == m_)))
    req.append(("attn_head_kernel, one head per workgroup at kvMul 16", has(lambda f, h, m, kv: m == 16 and has_head_kernel(h) and bd_group(h, m) == 1)))
    req.append(("qwen3 qk-norm at head size 160", has(lambda f, h, m, kv: (f, h) == ("qwen3", 160))))
    req.append(("qwen3 qk-norm at head size 256", has(lambda f, h, m, kv: (f, h) == ("qwen3", 256))))
    req.append(("qwen2 bias at head size 192", has(lambda f, h, m, kv: (f, h) == ("qwen2", 192))))
    req.append(("phi3 rope layout at head size 224", has(lambda f, h, m, kv: (f, h) == ("phi3", 224))))
    req.append(("granite attention scale at head size >= 160", has(lambda f, h, m, kv: f == "granite" and h >= 160)))
    for f_ in sorted(set(FAMILY.values())):
        req.append(("family %s" % f_, has(lambda f, h, m, kv: f == f_)))
    single = _shapes(names, lambda f, h, m, kv: kv == 1)
    req.append(("exactly one shape with a single kv head", len(single) == 1))
    return [what for what, ok in req if not ok]
