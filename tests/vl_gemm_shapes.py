"""The batched GEMM of the f32-activation weight types (csrc/gl3_prefill_vl.h): the rule by which launch_gemm_vl picks a kernel, its tiles
and its grid, restated in Python, and the grid of shapes that reaches every branch of it.

Every case is a Llama-architecture model of 2 layers, 8 query heads on 2 kv heads of 32 elements (q_dim 256, qkv 384 rows; n_heads *
head_size need not be dim, as in k_shapes.py); dim, hidden and vocab vary.  A step is the number of tokens of one prefill chunk ("chunk"
cases) or the number of output rows of a static-batched decode step / a mixed step with every row flagged ("rows" case).  The weight types
are q4v256 (Q4_0, K in chunks of 256) and q8f32 (Q8_0 with the f32 activation, chunks of 128) everywhere; f16v256 / f16v512 run where a row
of the grid lists them: their kernels take no part in the 192 rule but share the row and token tails and vl_tile_of.

The rule (vl_gemm_plan, gl3_prefill_vl.h):
    F16                  gemm_f16_mfma_kernel (512-bit species: gemm_f16_mfma_v512_kernel), 64 x 64 tiles, vl_tile_of
    Q4_0 / Q8_0-f32act   gemm_vlq_mfma_kernel (64 x 64 tiles; vqm_tile_of with G token groups and P = 8 / G row parts) when ntok > 16 and
                         ceil(rows / 64) * ceil(ntok / 64) >= 192; gemm_vlq_kernel (64 rows x 16 tokens, vl_tile_of) otherwise
    switches             GL3_VLQ_MFMA=0 (always gemm_vlq_kernel), GL3_VQM_XCD_TOKENS=0 (vl_tile_of on the matrix-pipe kernel),
                         GL3_VLQ_MFMA_MIN_TILES=<t> (t replaces 192), GL3_VQM_OCC2=1 (another build of the same kernel: no change of the plan)
tests/test_vl_gemm_shapes.py holds the rule to the library's own answer (gl3_debug_vl_gemm_plan) and asserts what the grid covers;
tests/test_gpu_vl_gemm_shapes.py runs the grid against the oracle."""

VLQ_TOK, VQM_TOK, F16G_TOK, TILE_ROWS, MIN_TILES = 16, 64, 64, 64, 192
KERNELS = ["gemm_f16_mfma_kernel", "gemm_f16_mfma_v512_kernel", "gemm_vlq_kernel", "gemm_vlq_mfma_kernel"]
VALU, MFMA = KERNELS[2], KERNELS[3]

#         kind       weight type, plan flags, oracle (vector_bits, f32_activation), elements of one VL chunk, legal step of an inner dimension
KINDS = {
    "q4v256":  dict(wtype=2, flags=(), oracle=(256, False), chunk=256, step=256),
    "q8f32":   dict(wtype=8, flags=("FLAG_F32_ACTIVATION",), oracle=(256, True), chunk=128, step=128),
    "f16v256": dict(wtype=1, flags=(), oracle=(256, False), chunk=64, step=64),
    "f16v512": dict(wtype=1, flags=("FLAG_VECTOR_512",), oracle=(512, False), chunk=64, step=64),
}
BLOCK_KINDS, F16_KINDS = ("q4v256", "q8f32"), ("f16v256", "f16v512")
HEADS, KV_HEADS, HEAD_SIZE, LAYERS = 8, 2, 32, 2
Q_DIM, QKV_ROWS = HEADS * HEAD_SIZE, (HEADS + 2 * KV_HEADS) * HEAD_SIZE
GRANITE = dict(embedding_scale=12.0, attention_scale=0.015625, residual_scale=0.22, logit_scale=8.0)      # tiny-granite's


# ---- the rule
def ceil_div(a, b):
    return (a + b - 1) // b


def vqm_groups(ntt):
    return 8 if ntt >= 8 else 4 if ntt >= 4 else 2 if ntt >= 2 else 1


def vqm_grid(nrt, ntt):
    g = vqm_groups(ntt)
    p = 8 // g
    return 8 * ceil_div(nrt, p) * ceil_div(ntt, g)


def vqm_tile_of(bid, nrt, ntt):
    """(row tile, token tile) of workgroup bid, or None: XCD x = bid & 7 works on token tiles x % G + G i and row tiles x // G + P j"""
    g = vqm_groups(ntt)
    p = 8 // g
    x, slot = bid & 7, bid >> 3
    nrp = ceil_div(nrt, p)
    rt, tt = x // g + p * (slot % nrp), x % g + g * (slot // nrp)
    return (rt, tt) if rt < nrt and tt < ntt else None


def vl_tile_of(bid, nrt, ntt):
    """the token tiles of one row tile take consecutive slots of one XCD"""
    per_xcd = (ntt * nrt + 7) >> 3
    j = (bid & 7) * per_xcd + (bid >> 3)
    return (j // ntt, j % ntt) if j < ntt * nrt else None


def plan(kind, rows, ntok, mfma=True, xcd_tokens=True, min_tiles=MIN_TILES):
    """What gl3_debug_vl_gemm_plan answers: kernel, row tiles, token tiles, grid, tile mapping, G, P"""
    nrt = ceil_div(rows, TILE_ROWS)
    if kind in F16_KINDS:
        ntt = ceil_div(ntok, F16G_TOK)
        return dict(kernel=KERNELS[1 if kind == "f16v512" else 0], nrt=nrt, ntt=ntt, grid=8 * ceil_div(nrt * ntt, 8), xcd_tokens=0, G=0, P=0)
    if ntok > VLQ_TOK and mfma and nrt * ceil_div(ntok, VQM_TOK) >= min_tiles:
        ntt = ceil_div(ntok, VQM_TOK)
        if xcd_tokens:
            g = vqm_groups(ntt)
            return dict(kernel=MFMA, nrt=nrt, ntt=ntt, grid=vqm_grid(nrt, ntt), xcd_tokens=1, G=g, P=8 // g)
        return dict(kernel=MFMA, nrt=nrt, ntt=ntt, grid=8 * ceil_div(nrt * ntt, 8), xcd_tokens=0, G=0, P=0)
    ntt = ceil_div(ntok, VLQ_TOK)
    return dict(kernel=VALU, nrt=nrt, ntt=ntt, grid=8 * ceil_div(nrt * ntt, 8), xcd_tokens=0, G=0, P=0)


def tiles(pl):
    """per workgroup of the plan's grid: its (row tile, token tile), or None for a workgroup that leaves at once"""
    of = vqm_tile_of if pl["xcd_tokens"] else vl_tile_of
    return [of(b, pl["nrt"], pl["ntt"]) for b in range(pl["grid"])]


def live_halves(ntok, tt):
    """gemm_vlq_mfma_kernel: which 32-token halves of token tile tt compute (a half past the end only helps staging)"""
    return tuple(tt * VQM_TOK + th * 32 < ntok for th in (0, 1))


def last_tile_tokens(ntok, tok=VQM_TOK):
    return ntok - tok * (ceil_div(ntok, tok) - 1)


def tail_class(ntok):
    """the token tail of a 64-token tile by what the kernel does with it"""
    t = last_tile_tokens(ntok)
    return {1: "1", 32: "32", 33: "33", 64: "64"}.get(t, "2..31" if t < 32 else "34..63")


# ---- the cases.  mode "chunk": steps are prefill chunks from position 0; mode "rows": output rows of static-batched decode steps ("bN": N
# sequences at depths 1 .. 3) and of mixed steps with every row flagged ("mN": one run of N rows)
CASES = {
    "resid":         dict(dim=3072, hidden=256, vocab=96, batch=256, mode="chunk", kinds=BLOCK_KINDS),
    "resid-granite": dict(dim=3072, hidden=256, vocab=96, batch=256, mode="chunk", kinds=("q4v256",), granite=True),
    "store":         dict(dim=512, hidden=3072, vocab=96, batch=256, mode="chunk", kinds=BLOCK_KINDS),
    "g8":            dict(dim=1536, hidden=256, vocab=96, batch=513, mode="chunk", kinds=BLOCK_KINDS),
    # 12304 = 192 * 64 + 16: the smallest row count above 12288 that gl3_create accepts (vocab % 16 == 0; 12296 is refused) and 64 does not divide
    "rows":          dict(dim=256, hidden=256, vocab=12304, batch=129, mode="rows", kinds=BLOCK_KINDS),
}
#  (case, step) -> the F16 species that run the row as well
GRID = {}


def _rows(case, steps, f16=()):
    for s in steps:
        GRID["%s-%s" % (case, s)] = dict(case=case, step=s, kinds=CASES[case]["kinds"] + (tuple(F16_KINDS) if s in f16 else ()))


_rows("resid", [192, 193, 224, 225, 256], f16=[193])
_rows("resid-granite", [193])
_rows("store", [192, 193])
_rows("g8", [448, 449, 512, 513])
_rows("rows", ["b16", "b17", "b32", "b33", "b64", "m65", "m129"], f16=["b33", "m65"])
FORM_ROWS = ["resid-193", "store-193", "g8-449", "rows-b33", "rows-m65"]      # one default-MFMA step per case for the A/B switches


def ntok_of(step):
    return int(step[1:]) if isinstance(step, str) else step


def ctx_of(case):
    """a multiple of 4, at least 64 beyond the deepest step"""
    deepest = max(ntok_of(r["step"]) for r in GRID.values() if r["case"] == case)
    return (deepest + 64 + 3) & ~3


def case_config(synth, case):
    c = CASES[case]
    extra = dict(GRANITE) if c.get("granite") else {}
    return synth.ModelConfig("vl-" + case, synth.ARCH_GRANITE if c.get("granite") else synth.ARCH_LLAMA, c["dim"], c["hidden"], LAYERS, HEADS, KV_HEADS,
                             HEAD_SIZE, c["vocab"], ctx_of(case), 1e-5, 500000.0, False, **extra)


def case_model(pkg, case, kind, seed=43):
    return pkg.synth.make_numpy(case_config(pkg.synth, case), wtype=KINDS[kind]["wtype"], seed=seed)


def kind_flags(hip, kind):
    f = 0
    for n in KINDS[kind]["flags"]:
        f |= getattr(hip, n)
    return f


def launches(name):
    """The GEMM launches of one layer and of the logits stage of a grid row: (projection, epilogue, rows, K, ntok, out_scale != 1).  A prefill
    chunk has no logits stage; the decode step behind it is a one-row step (gemm_vlq_kernel) and not listed."""
    r = GRID[name]
    c = CASES[r["case"]]
    n, scaled = ntok_of(r["step"]), bool(c.get("granite"))
    out = [("qkv", "store", QKV_ROWS, c["dim"], n, False), ("wo", "resid", c["dim"], Q_DIM, n, scaled), ("gate", "store", c["hidden"], c["dim"], n, False),
           ("up", "store", c["hidden"], c["dim"], n, False), ("down", "resid", c["dim"], c["hidden"], n, scaled)]
    if c["mode"] == "rows":
        out.append(("logits", "store", c["vocab"], c["dim"], n, scaled))
    return out


def facts(names):
    """What the block-format launches of the rows `names` reach, as a set of tuples"""
    have = set()
    for name in names:
        for kind in GRID[name]["kinds"]:
            for proj, epi, rows, k, ntok, scaled in launches(name):
                pl = plan(kind, rows, ntok)
                if kind in F16_KINDS:
                    have.add(("f16", kind, "token tail" if ntok % F16G_TOK else "full", "row tail" if rows % TILE_ROWS else "full"))
                    continue
                nrt, t64 = pl["nrt"], ceil_div(ntok, VQM_TOK)
                if pl["kernel"] == VALU:
                    if ntok > VLQ_TOK and nrt * (t64 + 1) >= MIN_TILES:
                        have.add(("below", epi, kind, t64 + 1))                 # one more token tile and the launch crosses
                    if ntok == VLQ_TOK and nrt >= MIN_TILES:
                        have.add(("16 tokens stay", kind))
                    continue
                g, ntt = pl["G"], pl["ntt"]
                if plan(kind, rows, ntok - 1)["kernel"] == VALU:
                    have.add(("at", epi, kind, ntt))                            # one token fewer and the launch stays behind
                have |= {("G", kind, g), ("tail", epi, kind, g, tail_class(ntok)), ("groups", kind, g, "ragged" if ntt % g else "full")}
                if rows % TILE_ROWS:
                    have.add(("cut row tile", kind, "inside" if rows % 16 else "between", "16-row MFMA tiles"))
                if nrt % pl["P"]:
                    have.add(("row parts ragged", kind))
                if k == KINDS[kind]["chunk"]:
                    have.add(("single chunk", kind))
                elif k == 2 * KINDS[kind]["chunk"]:
                    have.add(("two chunks", epi, kind))
                if scaled:
                    have.add(("out_scale", epi, kind))
                if not all(live_halves(ntok, ntt - 1)):
                    have.add(("dead half", kind))
    return have


def wanted():
    req = []
    for kind in BLOCK_KINDS:
        req += [("below", "resid", kind, 4), ("at", "resid", kind, 4), ("below", "store", kind, 4), ("at", "store", kind, 4),      # both sides of 192
                ("below", "resid", kind, 8), ("at", "resid", kind, 8), ("16 tokens stay", kind), ("at", "store", kind, 1)]
        req += [("G", kind, g) for g in (1, 2, 4, 8)]
        req += [("tail", "resid", kind, 4, t) for t in ("1", "32", "33", "64")] + [("tail", "resid", kind, 8, t) for t in ("1", "64")]
        req += [("tail", "store", kind, 1, t) for t in ("2..31", "32", "33", "64")] + [("tail", "store", kind, 2, "1")]
        req += [("groups", kind, g, f) for g in (2, 8) for f in ("full", "ragged")]
        req += [("cut row tile", kind, "between", "16-row MFMA tiles"), ("row parts ragged", kind), ("dead half", kind), ("two chunks", "store", kind)]
    # K of one VL chunk: q_dim / hidden 256 is one Q4_0 chunk; the Q8_0 chunk of 128 is below every legal wo / down K of these heads
    req += [("single chunk", "q4v256"), ("two chunks", "resid", "q8f32"), ("out_scale", "resid", "q4v256")]
    for kind in F16_KINDS:
        req += [("f16", kind, "token tail", "full"), ("f16", kind, "token tail", "row tail")]
    return req


def missing(names):
    """Requirements that the rows `names` do not meet (empty: the grid covers everything)"""
    have = facts(names)
    return [w for w in wanted() if w not in have]
