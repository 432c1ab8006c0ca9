"""The Q8_0 GEMMs of a batched step of more than 64 rows (pf_gemm3_kernel, csrc/gl3_prefill_gemm3.h; pf_gemm3t_kernel, gl3_prefill_gemm3t.h):
the rule by which g3_plan (csrc/gl3_prefill_gemm3.hip) picks a kernel, its workgroup tile and its grid, restated in Python, and the grid of
shapes that reaches every branch of it at the edges the kernels are built around.

Every case is a Llama-architecture model of 2 layers, 8 query heads on 2 kv heads of 32 elements (q_dim 256, qkv 384 rows; n_heads *
head_size need not be dim, as in k_shapes.py), Q8_0 with the int8 activation; dim, hidden and vocab vary, one case is Granite's (out_scale on
the residual and the logits launches).  A step is the number of tokens of one prefill chunk from position 0 ("chunk" cases) or "mNfF": a
mixed step of one run of N rows whose last F rows are flagged, so the logits launch has F output rows ("rows" cases).

The rule (g3_plan):
    store / resid   128 x 128 tiles (KB 2) when ceil(rows / 128) * ntt >= 512, 96 x 128 (KB 4) when rows % 96 == 0 and
                    128 < ceil(rows / 96) * ntt <= 384, else 64 x 128 (KB 4); ntt = ceil(ntok / 128)
    gate + up       the fewest tile-steps per SIMD between 128 x 128 (64 + 64 rows, KB 2; ceil(ntt * ceil(rows / 64) / 512) * 8) and the
                    tall tiling of NFR = 4 .. 7 row fragments (32 NFR rows per matrix, KB 2; ceil(ntt * ceil(rows / 32 NFR) / 256) * 2 NFR),
                    the first of equal costs: NFR 4 never costs less than 128 x 128 (2 ceil(r / 128) >= ceil(r / 64)), so only the switch reaches it
    hb quantised    by the gate + up launch itself when it is tall, KB 2 and rows % 32 == 0
    grid            tiles rounded up to 8; workgroup lin works on tile J = (lin & 7) * (grid / 8) + (lin >> 3) = (J / ntt, J % ntt)
    switches        GL3_PF_GEMM3_TALL=-1|4..7, GL3_PF_GEMM3_TALL_KB=1, GL3_PF_GEMM3_SHAPE=1|2|3|4 (4: 64 x 64 tiles, KB 4), GL3_PF_GEMM3_QOUT=0
What the step does around a launch (gl3_prefill.hip): a step of at most 64 rows, and a logits stage of at most 64 output rows inside a
longer step, run bdw_gemm_kernel on the XQ2 operand layout instead; these launches read the chunk-major one.
tests/test_gemm3_shapes.py holds the rule to the library's own answer (gl3_debug_gemm3_plan) and asserts what the grid covers;
tests/test_gpu_gemm3_shapes.py runs the grid and EDGE_CASES against the oracle; tests/test_gpu_gemm_forms.py repeats FORM_ROWS under the switches."""

KERNELS = ["pf_gemm3_kernel", "pf_gemm3t_kernel"]
G3, G3T = KERNELS
RING = 3                                               # K stages in flight (G3_RING)
HEADS, KV_HEADS, HEAD_SIZE, LAYERS = 8, 2, 32, 2
Q_DIM, QKV_ROWS = HEADS * HEAD_SIZE, (HEADS + 2 * KV_HEADS) * HEAD_SIZE
GRANITE = dict(embedding_scale=12.0, attention_scale=0.015625, residual_scale=0.22, logit_scale=8.0)      # tiny-granite's
TAILS = (1, 32, 33, 64, 65, 96, 97, 128)               # tokens of the last 128-token tile that change which 32-token columns are live


# ---- the rule
def ceil_div(a, b):
    return (a + b - 1) // b


def tall_cost(rows, ntok, nfr):
    """tile-steps per SIMD of the gate + up launch: nfr 0 = the 128 x 128 tiling"""
    ntt = ceil_div(ntok, 128)
    if nfr == 0:
        return ceil_div(ntt * ceil_div(rows, 64), 512) * 8
    return ceil_div(ntt * ceil_div(rows, 32 * nfr), 256) * 2 * nfr


def tall_choice(rows, ntok, tall=0):
    """g3_tall_choice: 0 = 128 x 128, 4 .. 7 = tall with that many row fragments"""
    best, cost = 0, tall_cost(rows, ntok, 0)
    if tall == 0:
        for nfr in (4, 5, 6, 7):
            if tall_cost(rows, ntok, nfr) < cost:
                best, cost = nfr, tall_cost(rows, ntok, nfr)
    return tall if 4 <= tall <= 7 else best


def plan(epi, rows, ntok, tall=0, tall_kb=2, shape=0, qout=True):
    """What gl3_debug_gemm3_plan answers.  epi: "store" | "resid" | "swiglu" (rows = hidden)"""
    p = dict(kernel=G3, tile_rows=64, tile_tok=128, KB=4, NFR=0, ntt=ceil_div(ntok, 128), qout=0)
    if epi == "swiglu":
        p["NFR"] = tall_choice(rows, ntok, tall)
        p["KB"] = 2
        if p["NFR"]:
            p.update(kernel=G3T, tile_rows=32 * p["NFR"], KB=1 if tall_kb == 1 else 2, qout=int(qout and tall_kb == 2 and rows % 32 == 0))
    else:
        t128, t96 = p["ntt"] * ceil_div(rows, 128), p["ntt"] * ceil_div(rows, 96)
        s = shape or (1 if t128 >= 512 else 2 if rows % 96 == 0 and 128 < t96 <= 384 else 3)
        if s == 1:
            p.update(tile_rows=128, KB=2)
        elif s == 2:
            p.update(tile_rows=96)
        elif s == 4:
            p.update(tile_tok=64, ntt=ceil_div(ntok, 64))
    p["nrt"] = ceil_div(rows, p["tile_rows"])
    p["grid"] = 8 * ceil_div(p["nrt"] * p["ntt"], 8)
    return p


def tile_of(lin, nrt, ntt):
    """(row tile, token tile) of workgroup lin, or None: the token tiles of one row tile take consecutive slots of one XCD"""
    per_xcd = (ntt * nrt + 7) >> 3
    j = (lin & 7) * per_xcd + (lin >> 3)
    return (j // ntt, j % ntt) if j < ntt * nrt else None


def tiles(pl):
    """per workgroup of the plan's grid: its (row tile, token tile), or None for a workgroup that leaves at once"""
    return [tile_of(b, pl["nrt"], pl["ntt"]) for b in range(pl["grid"])]


def tile_name(epi, pl):
    if pl["kernel"] == G3T:
        return "tall"
    return "%s%dx%d" % ("swiglu " if epi == "swiglu" else "", 2 * pl["tile_rows"] if epi == "swiglu" else pl["tile_rows"], pl["tile_tok"])


def stages(k, kb):
    """(K stages that hold a real block, real blocks of the last one)"""
    nb = k // 32
    return ceil_div(nb, kb), nb - kb * (ceil_div(nb, kb) - 1)


def last_tile_tokens(ntok, tok=128):
    return ntok - tok * (ceil_div(ntok, tok) - 1)


# ---- the cases.  mode "chunk": steps are prefill chunks from position 0; mode "rows": mixed steps "mNfF"
CASES = {
    # 64 x 128 and the 128 x 128 SwiGLU tiling at every token tail, one token tile and several; K of 5 blocks (qkv, KB 4: two stages, one real
    # block in the last, behind the 9 blocks the down projection's operand wrote; gate + up, KB 2: three stages, one real block in the last),
    # 8 (wo: two whole stages) and 9 (down: three stages); dim 160 cuts the last 64-row tile of wo / down to 32 rows, hidden 288 the last
    # 64 + 64 rows of gate + up to 32 + 32
    "tails":    dict(dim=160, hidden=288, vocab=96, batch=256, mode="chunk"),
    # one K stage everywhere but wo: dim 32 = one block (KB 4 and KB 2), hidden 96 = three blocks of one stage; fewer stages than the ring
    "k1":       dict(dim=32, hidden=96, vocab=96, batch=130, mode="chunk"),
    # dim 96: one stage of three blocks (KB 4), two stages with one real block in the last (KB 2); hidden 192: two stages, two real blocks
    "k2":       dict(dim=96, hidden=192, vocab=96, batch=130, mode="chunk"),
    # dim 224: two stages with three real blocks in the last (KB 4), four stages with one (KB 2); hidden 416: four stages, one real block
    "k4":       dict(dim=224, hidden=416, vocab=96, batch=130, mode="chunk"),
    # dim 384: three whole stages (KB 4), six (KB 2), the ring wraps twice; hidden 512: four whole stages
    "k3":       dict(dim=384, hidden=512, vocab=96, batch=130, mode="chunk"),
    # tall by default at 385 .. 512 tokens: NFR 5 (last row tile 2 of 5 fragments), 6 (3 of 6), 7 (whole tiles), and hidden 14368 (2048 rows
    # further): back to 128 x 128.  dim 160 / 64 / 128: the tall kernel with three K stages and one real block in the last, with one, with
    # two.  hb leaves gate + up quantised, and hidden % 128 = 32: the down projection's last stage reads three blocks that only
    # gl3_prefill_alloc ever wrote
    "tall5":    dict(dim=160, hidden=8224, vocab=96, batch=512, mode="chunk"),
    "tall6":    dict(dim=64, hidden=10272, vocab=96, batch=512, mode="chunk"),
    "tall7":    dict(dim=128, hidden=12320, vocab=96, batch=512, mode="chunk"),
    "tall-end": dict(dim=64, hidden=14368, vocab=96, batch=512, mode="chunk"),
    # 96 x 128 by default on wo / down: 33 row tiles x 4 token tiles = 132; dim 3072 (32 x 4 = 128) is the last 64 x 128 shape below it,
    # and its qkv launch the longest K of the grid on whole stages (96 blocks: the ring of three wraps eight times)
    "r96":      dict(dim=3168, hidden=64, vocab=96, batch=512, mode="chunk", granite=True),
    "r96-below": dict(dim=3072, hidden=64, vocab=96, batch=512, mode="chunk"),
    # the logits launch (store): vocab 12384 = 129 x 96 rows takes 96 x 128 at 65 .. 256 flagged rows (129 / 258 tiles) and 64 x 128 at 257
    # (387 tiles), and 64 or fewer flagged rows leave for bdw_gemm_kernel inside a step of more than 64 rows
    "s96":      dict(dim=32, hidden=32, vocab=12384, batch=257, mode="rows", granite=True),
    # 128 x 128 by default for store: 32672 rows = 256 row tiles, the last one of 32 rows; 129 flagged rows make 512 tiles, 128 do not;
    # 161: the last token tile keeps two of its four 32-token fragments
    "s128":     dict(dim=32, hidden=32, vocab=32672, batch=161, mode="rows"),
}
# The edge-VALUE models of tests/edge_models.py ("all" edits: zero, f16-subnormal, rounds-to-zero and outlier activation blocks, zero /
# subnormal / negative / large weight scales, quants at -128 and +-127, peaked attention) at shapes that take the tall kernel and the
# 96 x 128 tile by default; the edits are laid out for dim of 8 blocks or more and hidden of 8 or more, so those stay at 256.
#   edge-tall   hidden 8224 at 385 tokens: NFR 5, hb quantised by the epilogue of pf_gemm3t_kernel.  inner-act-blocks makes the hb blocks
#               of rows 32 .. 191 (first and second row tile) zero, f16-subnormal in scale and ordinary beside them
#   edge-r96    dim 3168 at 385 tokens: wo / down on 96 x 128 with Granite's out_scale, the act-blocks of 99 K blocks into qkv / gate + up
EDGE_CASES = {
    "edge-tall": dict(cfg="tiny-llama", dim=256, hidden=8224, step=385),
    "edge-r96":  dict(cfg="tiny-granite", dim=3168, hidden=256, step=385),
}
GRID = {}


def _rows(case, steps):
    for s in steps:
        GRID["%s-%s" % (case, s)] = dict(case=case, step=s)


_rows("tails", [65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256])
_rows("k1", [65, 130])
_rows("k2", [65, 130])
_rows("k4", [65, 130])
_rows("k3", [65, 130])
_rows("tall5", [385, 416, 417, 448, 449, 480, 481, 512])
_rows("tall6", [385, 512])
_rows("tall7", [385, 512])
_rows("tall-end", [385, 512])
_rows("r96", [385, 416, 417, 448, 449, 480, 481, 512])
_rows("r96-below", [385, 512])
_rows("s96", ["m65f64", "m65f65", "m96f96", "m97f97", "m128f128", "m257f64", "m257f65", "m257f129", "m257f256", "m257f257"])
_rows("s128", ["m129f128", "m129f129", "m161f161"])
# Rows repeated under the switches (tests/test_gpu_gemm_forms.py): every tile shape the defaults of this grid do not reach on that epilogue.
# The 128 x 128 tile on the RESIDUAL epilogue runs only here, under GL3_PF_GEMM3_SHAPE=1: by default it needs dim >= 10912 at 641 or more
# tokens, and the oracle's run of such a case takes far longer than the few seconds a test may.  By default the plain 128 x 128 tile runs on
# the store epilogue alone (s128), where its last token tile holds 1 or 33 tokens behind a full one; under SHAPE=1 these rows give it every
# tail of TAILS, with one token tile (65, 97) and with several (1, 32, 33, 64, 96, 128), on wo / down / qkv of the tails case.
FORM_ROWS = ["tails-65", "tails-97", "tails-129", "tails-160", "tails-161", "tails-192", "tails-224", "tails-256", "k1-130", "k4-130", "tall5-385",
             "s96-m97f97"]


def ntok_of(step):
    """(rows of the step, output rows of its logits launch; 0: a chunk has none)"""
    if isinstance(step, str):
        n, f = step[1:].split("f")
        return int(n), int(f)
    return step, 0


def ctx_of(case):
    """a multiple of 4, at least 64 beyond the deepest step"""
    deepest = max(ntok_of(r["step"])[0] for r in GRID.values() if r["case"] == case)
    return (deepest + 64 + 3) & ~3


def case_config(synth, case):
    c = CASES[case]
    extra = dict(GRANITE) if c.get("granite") else {}
    return synth.ModelConfig("g3-" + case, synth.ARCH_GRANITE if c.get("granite") else synth.ARCH_LLAMA, c["dim"], c["hidden"], LAYERS, HEADS, KV_HEADS,
                             HEAD_SIZE, c["vocab"], ctx_of(case), 1e-5, 500000.0, False, **extra)


def case_model(pkg, case, seed=47):
    return pkg.synth.make_numpy(case_config(pkg.synth, case), wtype=8, seed=seed)


def edge_model(case):
    """The "all" model of edge_models.py at the case's dim / hidden (2 layers, 8 query heads on 2 kv heads of 32, as every case here)"""
    import edge_models as em
    c = EDGE_CASES[case]
    return em.make_edge_model(c["cfg"], 8, 7, "all", dim=c["dim"], hidden=c["hidden"], ctx=(c["step"] + 64 + 3) & ~3)


def edge_tokens(pkg, m, n):
    """edge_models.edge_tokens, and the zero and the flat token again on both sides of the first token-tile boundary and at the end of the
    chunk: with n = 385 the zero token is the only row of the last token tile"""
    import edge_models as em
    t = em.edge_tokens(pkg, m, n + 1)
    for p, tok in ((126, em.FLAT_TOKEN), (127, em.ZERO_TOKEN), (128, em.ZERO_TOKEN), (129, em.FLAT_TOKEN), (n - 2, em.FLAT_TOKEN), (n - 1, em.ZERO_TOKEN)):
        t[p] = tok
    return t


def edge_launches(case):
    c = EDGE_CASES[case]
    n = c["step"]
    return [("qkv", "store", QKV_ROWS, c["dim"], n), ("wo", "resid", c["dim"], Q_DIM, n), ("gate+up", "swiglu", c["hidden"], c["dim"], n),
            ("down", "resid", c["dim"], c["hidden"], n)]


def launches(name):
    """The > 64-token GEMM launches of one layer and of the logits stage of a grid row: (projection, epilogue, rows, K, ntok, out_scale != 1).
    A logits stage of at most 64 output rows is no launch of these kernels and not listed."""
    r = GRID[name]
    c = CASES[r["case"]]
    (n, f), scaled = ntok_of(r["step"]), bool(c.get("granite"))
    out = [("qkv", "store", QKV_ROWS, c["dim"], n, False), ("wo", "resid", c["dim"], Q_DIM, n, scaled),
           ("gate+up", "swiglu", c["hidden"], c["dim"], n, False), ("down", "resid", c["dim"], c["hidden"], n, scaled)]
    if f > 64:
        out.append(("logits", "store", c["vocab"], c["dim"], f, scaled))
    return out


def maxk_of(case):
    c = CASES[case]
    return (max(c["dim"], c["hidden"], Q_DIM) + 127) & ~127


def facts(names):
    """What the launches of the rows `names` reach, as a set of tuples"""
    have = set()
    for name in names:
        c = CASES[GRID[name]["case"]]
        n, f = ntok_of(GRID[name]["step"])
        ls = launches(name)
        if c["mode"] == "rows":
            have.add(("logits stage", "step of %d rows" % n, "64 or fewer rows" if f <= 64 else "65 rows" if f == 65 else
                      "ragged above 128" if f > 128 and f % 128 else "other"))
        for proj, epi, rows, k, ntok, scaled in ls:
            pl = plan(epi, rows, ntok)
            tn = tile_name(epi, pl)
            have.add(("default", epi, tn) + ((pl["NFR"],) if tn == "tall" else ()))
            # a token tail is held on a launch of a named K: ragged last stages and dead token columns meet in the same workgroup
            have.add(("tail", tn, "K blocks", k // 32, "one token tile" if pl["ntt"] == 1 else "several", last_tile_tokens(ntok)))
            nst, real = stages(k, pl["KB"])
            have.add(("stages", pl["KB"], min(nst, 5)))
            # and a shape of the K loop (stages, 5 = five or more; real blocks of the last) with one token tile and with several
            have.add(("K loop", epi, tn, min(nst, 5), real, "one token tile" if pl["ntt"] == 1 else "several"))
            if tn == "tall":
                have.add(("tall stages", min(nst, 4), real))
            if real < pl["KB"]:
                have.add(("last stage", pl["KB"], real))
            if rows % pl["tile_rows"]:
                have.add(("cut row tile", tn))
                if tn == "tall":
                    have.add(("tall live fragments", pl["NFR"], ceil_div(rows % pl["tile_rows"], 32)))
            elif tn == "tall":
                have.add(("tall whole tiles", pl["NFR"]))
            if pl["grid"] > pl["nrt"] * pl["ntt"]:
                have.add(("surplus workgroups", tn))
            if scaled:
                have.add(("out_scale", epi))
            if pl["qout"]:
                have.add(("hb quantised", "ragged last row tile" if rows % pl["tile_rows"] else "whole tiles"))
                if rows % 128:
                    have.add(("hb quantised", "blocks past hidden stay zero"))
            # both sides of every branch of the choice
            if epi == "swiglu":
                other = plan(epi, rows - 2048, ntok)
                if pl["NFR"] != other["NFR"]:
                    have.add(("NFR step", other["NFR"], pl["NFR"]))
            else:
                t128, t96 = pl["ntt"] * ceil_div(rows, 128), pl["ntt"] * ceil_div(rows, 96)
                if t128 in (511, 512):
                    have.add(("t128", epi, t128))
                if pl["tile_rows"] != 128 and plan(epi, rows, ntok + 1)["tile_rows"] == 128:
                    have.add(("one token more takes 128x128", epi))
                if rows % 96 == 0 and t96 in (128, 129, 132, 384, 385, 387):
                    have.add(("t96", epi, "128 or fewer" if t96 <= 128 else "just above 128" if t96 <= 132 else "384" if t96 == 384 else "above 384"))
        # a short K behind a longer one in the same operand buffer: the quantise launch of dim writes ceil(dim / 32) blocks where the
        # f32 hb of the layer before was quantised over hidden / 32, and the launch reads whole stages
        gu = plan("swiglu", c["hidden"], n)
        if not gu["qout"] and c["hidden"] > c["dim"] and (c["dim"] // 32) % 4:
            have.add(("short K behind a longer one",))
        if any(GRID[o]["case"] == GRID[name]["case"] and ntok_of(GRID[o]["step"])[0] > n for o in names):      # the longest step runs first
            have.add(("stale token slots", GRID[name]["case"]))
    return have


def wanted():
    req = [("default", "store", "64x128"), ("default", "store", "96x128"), ("default", "store", "128x128"),
           ("default", "resid", "64x128"), ("default", "resid", "96x128"), ("default", "swiglu", "swiglu 128x128")]
    req += [("default", "swiglu", "tall", nfr) for nfr in (5, 6, 7)]
    req += [("NFR step", 0, 5), ("NFR step", 5, 6), ("NFR step", 6, 7), ("NFR step", 7, 0)]
    # token tails: 64 x 128 and the 128 x 128 SwiGLU tiling with one token tile and several; 96 x 128 with several on the residual epilogue
    # and with one on the store epilogue; the tall kernel with several (one token tile is tall only under GL3_PF_GEMM3_TALL: hidden would
    # have to pass 32768, above the largest gl3_create accepts)
    # (on the down projection at 9 blocks, gate + up at 5, wo at 8, the logits launch at 1, tall gate + up at 5)
    for tn, nb in (("64x128", 9), ("swiglu 128x128", 5)):
        req += [("tail", tn, "K blocks", nb, "one token tile", t) for t in TAILS[4:]] + [("tail", tn, "K blocks", nb, "several", t) for t in TAILS]
    req += [("tail", "96x128", "K blocks", 8, "several", t) for t in TAILS] + [("tail", "96x128", "K blocks", 1, "one token tile", t) for t in TAILS[4:]]
    req += [("tail", "96x128", "K blocks", 1, "several", 1), ("tail", "96x128", "K blocks", 1, "several", 128)]
    req += [("tail", "tall", "K blocks", 5, "several", t) for t in TAILS]
    # NFR 6 (K of 2 blocks) and NFR 7 (4 blocks): the first and the last tail; the 128 x 128 SwiGLU tiling at 900 tiles (K of 2 blocks) and
    # 64 x 128 on the longest K (qkv at 96 blocks) likewise
    req += [("tail", tn, "K blocks", nb, "several", t) for tn, nb in (("tall", 2), ("tall", 4), ("swiglu 128x128", 2), ("64x128", 96)) for t in (1, 128)]
    # plain 128 x 128: one and two live 32-token fragments of the last token tile by default (the rest: FORM_ROWS under GL3_PF_GEMM3_SHAPE=1)
    req += [("tail", "128x128", "K blocks", 1, "several", 1), ("tail", "128x128", "K blocks", 1, "several", 33)]
    req += [("stages", kb, s) for kb in (2, 4) for s in (1, 2, 3, 4, 5)]
    # every shape of the K loop of k1 .. k4 under one token tile and under several (a ragged last stage and dead token columns in one workgroup)
    for mult in ("one token tile", "several"):
        req += [("K loop", "resid", "64x128", s, real, mult) for s, real in ((1, 3), (2, 2), (4, 1), (4, 4))]
        req += [("K loop", "store", "64x128", s, real, mult) for s, real in ((1, 1), (1, 3), (2, 3), (3, 4))]
        req += [("K loop", "swiglu", "swiglu 128x128", s, real, mult) for s, real in ((1, 1), (2, 1), (4, 1), (5, 2))]
    req += [("tall stages", 1, 2), ("tall stages", 2, 2), ("tall stages", 3, 1)]
    req += [("last stage", 4, 1), ("last stage", 4, 2), ("last stage", 4, 3), ("last stage", 2, 1)]
    req += [("cut row tile", tn) for tn in ("64x128", "swiglu 128x128", "tall", "128x128")]
    req += [("tall live fragments", 5, 2), ("tall live fragments", 6, 3), ("tall whole tiles", 7)]
    req += [("surplus workgroups", tn) for tn in ("64x128", "96x128", "swiglu 128x128", "tall")]
    req += [("out_scale", "resid"), ("out_scale", "store")]
    req += [("hb quantised", "ragged last row tile"), ("hb quantised", "whole tiles"), ("hb quantised", "blocks past hidden stay zero")]
    req += [("t128", "store", 512), ("one token more takes 128x128", "store"), ("t96", "resid", "128 or fewer"), ("t96", "resid", "just above 128"),
            ("t96", "store", "just above 128"), ("t96", "store", "above 384")]
    # the three logits stages of the SAME step of 257 rows, and the first two on the shortest step of these kernels
    req += [("logits stage", "step of 257 rows", k) for k in ("64 or fewer rows", "65 rows", "ragged above 128")]
    req += [("logits stage", "step of 65 rows", k) for k in ("64 or fewer rows", "65 rows")]
    req += [("short K behind a longer one",)]
    req += [("stale token slots", case) for case in CASES]        # every case: a shorter step over the token slots of a longer one
    return req


def missing(names):
    """Requirements that the rows `names` do not meet (empty: the grid covers everything)"""
    have = facts(names)
    return [w for w in wanted() if w not in have]
