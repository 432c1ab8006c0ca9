"""The Q8_0 GEMM of a batched step of at most 64 rows (bdw_gemm_kernel, csrc/gl3_bd_gemm.h; launched by launch_gemm, csrc/gl3_prefill.hip):
the rule by which bd_gemm_plan sizes a launch and bdw_place_unit / bdw_place_tile hand its workgroups their work, restated in Python, and the grid of shapes that
reaches every form of the kernel's K walk, of its grid and of its token tiles.

Every case is a Llama-architecture model of 2 layers, 8 query heads on 2 kv heads of 32 elements (q_dim 256, qkv 384 rows = 24 strips;
n_heads * head_size need not be dim, as in k_shapes.py), Q8_0 with the int8 activation, ctx 96; dim, hidden and vocab vary, one case is
Granite's (out_scale on the residual and the logits launches, scaled embedding and attention).

The rule:
    token slots     TS = 32 for a launch of at most 32 tokens, 64 up to 64, above that not this kernel (bd_tslots).  The logits launch of a
                    step takes the TS of its OUTPUT rows, the layers' launches the TS of the step's rows.
    DA              tiles (4 blocks = 128 elements of K) in flight: 8 for store / residual (qkv, wo, down, logits), 4 for SwiGLU (gate + up)
    K walk          nb = K / 32 blocks, nfull = nb >> 2 full tiles, ntiles = ceil(nb / 4); nfull / DA full trips of DA tiles without a
                    branch, then, when tiles are left, one partial trip that runs ntiles - trips * DA tiles; the last of them holds nb % 4
                    blocks when that is not 0.  The rings fetch DA tiles beyond the last one whatever K is.
    units           16-row strips; the quantising gate + up form (two wavefronts, 128 threads) takes 32-row strip pairs
    grid            units rounded up to 8, times the token tiles of 16: bdw_grid.  Workgroup id works on unit (id / (8 ntt)) * 8 + id % 8
                    and token tile (id / 8) % ntt (bdw_place_unit, bdw_place_tile) and leaves at once when that unit does not exist.
    fuse_q          on one rank with GL3_NO_FUSED_QUANT unset (hidden % 32 == 0 and head_size % 32 == 0 hold for every plan gl3_create
                    accepts) gate + up runs the quantising form and writes hb as the down projection's operand
    rows            gl3_create accepts only Q8_0 row counts that are multiples of 16 (dim % 32, hidden % 32, vocab % 16 on one rank;
                    dim / 16, hidden / 16 and vocab / 16 divisible by the rank count): the kernel's `rbase + i >= rows` guard is unreachable
                    and no row of the grid asks for it.  On ONE rank dim % 32 == 0, so a residual launch of 16 x an odd number of rows exists
                    only under tensor parallelism: case k3 on two ranks (dim / 2 = 48 rows = 3 strips).
A step is written (form, n): "chunk": a prefill chunk of n tokens from position 0 into a fresh sequence; "batch": a static-batched decode step
of the first n sequences, every one at its own depth below 128, logits and ids of every row; "mixed": one gl3_forward_batch of n rows (one
decode row and two runs; "mixed-all": every row an output row).
tests/test_bd_gemm_shapes.py holds the rule to the library's own answer (gl3_debug_bd_gemm_plan) and asserts what the grid covers;
tests/test_gpu_bd_gemm_shapes.py runs the grid against the oracle."""

BD_TS, BD_TS_MAX = 32, 64
TILE_BYTES = 2176                                      # one Q8T tile: 16 rows x 4 blocks
HEADS, KV_HEADS, HEAD_SIZE, LAYERS, CTX = 8, 2, 32, 2, 96
Q_DIM, QKV_ROWS = HEADS * HEAD_SIZE, (HEADS + 2 * KV_HEADS) * HEAD_SIZE
GRANITE = dict(embedding_scale=12.0, attention_scale=0.015625, residual_scale=0.22, logit_scale=8.0)      # tiny-granite's
COUNTS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)      # every edge of a 16-token tile up to 64
UNITS = (1, 7, 8, 9, 16, 17)                           # the grid pads to 8 units: one, one short of / on / past 8 and 16
EPIS = ("store", "resid", "swiglu")


# ---- the rule
def ceil_div(a, b):
    return (a + b - 1) // b


def tslots(n):
    return BD_TS if n <= BD_TS else BD_TS_MAX if n <= BD_TS_MAX else 0


def da_of(epi):
    return 4 if epi == "swiglu" else 8


def k_walk(k, da):
    """The K loop of a launch: blocks, full tiles, tiles, full trips, tiles of the partial trip, blocks of a ragged last tile (0: none)"""
    nb = k // 32
    nfull, ntiles = nb >> 2, ceil_div(nb, 4)
    trips = nfull // da
    return dict(nb=nb, nfull=nfull, ntiles=ntiles, trips=trips, partial=ntiles - trips * da, ragged=nb % 4)


def bdw_grid(units, ntt):
    return ceil_div(units, 8) * 8 * ntt


def place(wg, ntt, units):
    """(unit, token tile) of workgroup wg, or None: it exits"""
    unit, h = (wg // (8 * ntt)) * 8 + (wg & 7), (wg >> 3) % ntt
    return (unit, h) if unit < units else None


def fuse_q(n, hidden, head_size=HEAD_SIZE, ranks=1, no_fused_quant=False):
    return not no_fused_quant and tslots(n) != 0 and ranks == 1 and hidden % 32 == 0 and head_size % 32 == 0


def plan(epi, rows, k, ntok, qout=False, wg=-1):
    """What gl3_debug_bd_gemm_plan answers"""
    ts = tslots(ntok)
    if not ts:
        return dict(ts=0, DA=0, qout=0, threads=0, ntt=0, units=0, grid=0, ntiles=0, trips=0, partial=0, place=None)
    da, q = da_of(epi), int(epi == "swiglu" and qout)
    ntt, units, kw = ceil_div(ntok, 16), ceil_div(rows, 32 if q else 16), k_walk(k, da)
    grid = bdw_grid(units, ntt)
    return dict(ts=ts, DA=da, qout=q, threads=128 if q else 64, ntt=ntt, units=units, grid=grid, ntiles=kw["ntiles"], trips=kw["trips"],
                partial=kw["partial"], place=place(wg, ntt, units) if 0 <= wg < grid else None)


def ring_reach(k, da, ts):
    """Bytes from the start of a strip / of XQ2 / of XS2 to the end of the furthest load of a launch: the prologue fetches DA tiles and every
    tile the trips work on fetches one more, so the last fetch is tile DA + ntiles - 1; a weight fetch also loads the scale header of the
    tile behind it (lanes 32 - 63)"""
    last = da + k_walk(k, da)["ntiles"] - 1
    return dict(w=(last + 1) * TILE_BYTES + 128, xq=(last + 1) * ts * 128, xs=(last + 1) * ts * 16)


# ---- the cases: dim, hidden, vocab.  K of gate + up (DA 4), qkv and logits (DA 8) = dim; of down (DA 8) = hidden; of wo (DA 8) = 256
CASES = {
    # one tile of 1 .. 4 blocks: the prologue fetches DA - 1 tiles of slack and the only trip is partial.  hidden 32 / 224 / 256 / 288: the
    # quantising form on 1, 7, 8, 9 strip pairs; vocab 16 / 112 / 128 / 144: the plain form on 1, 7, 8, 9 strips
    "k1":  dict(dim=32, hidden=32, vocab=16),
    "k2":  dict(dim=64, hidden=224, vocab=112),
    "k3":  dict(dim=96, hidden=256, vocab=128),
    "k4":  dict(dim=128, hidden=288, vocab=144),
    # dim 384: DA - 1 = 3 tiles for gate + up; hidden 896: 7 tiles for down
    "k12": dict(dim=384, hidden=896, vocab=256),
    # dim 512 / hidden 1024: exactly DA full tiles, one full trip and no partial one
    "k16": dict(dim=512, hidden=1024, vocab=272),
    # DA full tiles and a ragged tile of 1, 2, 3 blocks alone in the partial trip, at slot 0 (dim for gate + up, hidden for down); k17 is Granite's
    "k17": dict(dim=544, hidden=1056, vocab=96, granite=True),
    "k18": dict(dim=576, hidden=1088, vocab=96),
    "k19": dict(dim=608, hidden=1120, vocab=96),
    # dim 992 = 31 blocks: the ragged tile in the last slot of the partial trip at both depths (nfull 7: DA 8 slot 7, DA 4 one full trip and
    # slot 3); an even tile count with a ragged end.  hidden 512: 16 strip pairs.  This case runs every token count in every form.
    "k31": dict(dim=992, hidden=512, vocab=96, every_count=True),
    # dim 2112 = 66 blocks: two full trips of 8 (four of 4) and a partial one of one ragged tile; 17 tiles (odd); hidden 544: 17 strip pairs
    "k66": dict(dim=2112, hidden=544, vocab=96),
}
TP_CASE = "k3"            # two in-process ranks: dim / 2 = 48 rows = 3 strips on wo / down (rank-chunked rows, no quantised hand-over)
# chunk sizes of one plan in this order: 65 (chunk-major operands in the same XQ) then 64 then 32 (both small layouts over them); 64 then 33
# then 64 (same TS, dead lanes in the last tile); 64 then 17 (the 32-slot layout over the 64-slot bytes)
STALE_ORDER = (65, 64, 32, 64, 33, 64, 17)
STALE = {"65>64>32": (65, 64, 32), "64>33>64": (64, 33, 64), "64>17": (64, 17)}


def steps_of(case):
    """The steps of a case in the order its plans run them: (form, n)"""
    more = [n for n in sorted(COUNTS, reverse=True) if n not in STALE_ORDER] if CASES[case].get("every_count") else []
    out = [("chunk", n) for n in list(STALE_ORDER) + more]
    out += [("batch", n) for n in [64, 17, 64, 33, 32] + more]
    out += [("mixed", 33), ("mixed-all", 32)] + [("mixed", n) for n in sorted(COUNTS, reverse=True) if n not in (32, 33) and (more or n == 64)]
    if more:
        out += [("mixed-all", 49), ("mixed", 32)]
    return out


def mixed_runs(n):
    """Row counts of a mixed step of n rows: (decode rows, [run lengths])"""
    if n < 3:
        return (n, []) if n == 1 else (0, [n])
    rest = n - 1
    return 1, ([ceil_div(rest, 2), rest // 2] if rest >= 4 else [rest])


def outputs_of(form, n):
    """Output rows of the step's logits stage (0: a chunk has none)"""
    if form == "chunk":
        return 0
    if form in ("batch", "mixed-all"):
        return n
    single, runs = mixed_runs(n)
    return single + len(runs)


def case_config(synth, case):
    c = CASES[case]
    extra = dict(GRANITE) if c.get("granite") else {}
    return synth.ModelConfig("bd-" + case, synth.ARCH_GRANITE if c.get("granite") else synth.ARCH_LLAMA, c["dim"], c["hidden"], LAYERS, HEADS, KV_HEADS,
                             HEAD_SIZE, c["vocab"], CTX, 1e-5, 500000.0, False, **extra)


def case_model(pkg, case, seed=53):
    return pkg.synth.make_numpy(case_config(pkg.synth, case), wtype=8, seed=seed)


def launches(case, form, n, ranks=1, no_fused_quant=False):
    """The bdw_gemm_kernel launches of one layer and of the logits stage of a step: (projection, epilogue, rows, K, ntok, qout).  A step of
    65 tokens has none in its layers."""
    c = CASES[case]
    dim, hid, f = c["dim"], c["hidden"], outputs_of(form, n)
    out = []
    if tslots(n):
        q = fuse_q(n, hid, ranks=ranks, no_fused_quant=no_fused_quant)
        out += [("qkv", "store", QKV_ROWS // ranks, dim, n, False), ("wo", "resid", dim // ranks, Q_DIM, n, False),
                ("gate+up", "swiglu", hid // ranks, dim, n, q), ("down", "resid", dim // ranks, hid, n, False)]
    if f and tslots(f):
        out.append(("logits", "store", c["vocab"] // ranks, dim, f, False))
    return out


def maxk_of(case):
    c = CASES[case]
    return (max(c["dim"], c["hidden"], Q_DIM) + 127) & ~127


def k_facts(da, k):
    """What the K walk of a launch is, as names"""
    w = k_walk(k, da)
    out = {("K", da, "odd tile count" if w["ntiles"] % 2 else "even tile count")}
    if w["nb"] <= 4:
        out.add(("K", da, "one tile of %d blocks" % w["nb"]))
    if w["ntiles"] == da - 1 and not w["ragged"]:
        out.add(("K", da, "DA - 1 tiles"))
    if w["nb"] == 4 * da:
        out.add(("K", da, "exactly DA full tiles"))
        assert w["trips"] == 1 and w["partial"] == 0
    if w["nfull"] == da and w["ragged"]:
        out.add(("K", da, "DA full tiles and a ragged one of %d blocks" % w["ragged"]))
        assert w["trips"] == 1 and w["partial"] == 1
    if w["ragged"] and w["nfull"] % da == da - 1:
        out.add(("K", da, "ragged tile in the last slot of the partial trip"))
        assert w["partial"] == da
    if w["trips"] >= 2 and w["partial"]:
        out.add(("K", da, "two full trips and a partial one"))
    return out


def facts(cases):
    """What the steps of the cases reach, as a set of tuples"""
    have = set()
    for case in cases:
        c = CASES[case]
        steps = steps_of(case)
        ragged = bool((c["dim"] // 32) % 4)
        if c["dim"] != Q_DIM:
            have.add(("a short K behind a longer one in the same operand",))
        if c.get("granite"):
            have.add(("out_scale, resid_scale and logit_scale != 1",))
        if (c["vocab"] // 16) % 2:
            have.add(("vocabulary of 16 x an odd number of rows",))
        if case == TP_CASE and (c["dim"] // 2) % 32 == 16:
            have.add(("residual launch of 16 x an odd number of rows", "two ranks"))
        for form, n in steps:
            kind = "mixed" if form.startswith("mixed") else form
            have.add(("tokens", case, n, kind))
            if ragged:
                have.add(("tokens on a ragged last K tile", n, kind))
            f = outputs_of(form, n)
            if kind == "mixed" and n >= 33 and 1 <= f <= 3:
                have.add(("mixed step", "body TS 64, logits TS 32"))
            if kind == "mixed" and n <= 32 and f == n:
                have.add(("mixed step", "n <= 32 and every row flagged"))
            for proj, epi, rows, k, ntok, q in launches(case, form, n):
                pl = plan(epi, rows, k, ntok, q)
                have |= k_facts(pl["DA"], k)
                have.add(("instantiation", epi, pl["DA"], bool(pl["qout"]), pl["ts"]))
                if pl["units"] in UNITS:
                    have.add(("units", "quantising" if pl["qout"] else "plain", pl["units"]))
        order = [n for form, n in steps if form == "chunk"]
        for name, seq in STALE.items():
            if any(tuple(order[i:i + len(seq)]) == seq for i in range(len(order))):
                have.add(("stale slots", case, name))
    return have


def wanted(cases=tuple(CASES)):
    req = []
    for da in (4, 8):
        req += [("K", da, "one tile of %d blocks" % b) for b in (1, 2, 3, 4)]
        req += [("K", da, "DA - 1 tiles"), ("K", da, "exactly DA full tiles")]
        req += [("K", da, "DA full tiles and a ragged one of %d blocks" % b) for b in (1, 2, 3)]
        req += [("K", da, "ragged tile in the last slot of the partial trip"), ("K", da, "two full trips and a partial one"),
                ("K", da, "odd tile count"), ("K", da, "even tile count")]
    req += [("a short K behind a longer one in the same operand",)]
    req += [("units", form, u) for form in ("plain", "quantising") for u in UNITS]
    req += [("vocabulary of 16 x an odd number of rows",), ("residual launch of 16 x an odd number of rows", "two ranks")]
    req += [("tokens on a ragged last K tile", n, kind) for n in COUNTS for kind in ("chunk", "batch", "mixed")]
    req += [("tokens", case, n, kind) for case in cases for n in (32, 33) for kind in ("chunk", "batch", "mixed")]
    req += [("mixed step", "body TS 64, logits TS 32"), ("mixed step", "n <= 32 and every row flagged")]
    req += [("stale slots", case, name) for case in cases for name in STALE]
    req += [("out_scale, resid_scale and logit_scale != 1",)]
    # every instantiation launch_gemm can launch on one rank by default
    req += [("instantiation", epi, 8, False, ts) for epi in ("store", "resid") for ts in (32, 64)]
    req += [("instantiation", "swiglu", 4, True, ts) for ts in (32, 64)]
    return req


def missing(cases):
    """Requirements that the cases do not meet (empty: the grid covers everything).  The per-case requirements (32 | 33 tokens and the stale
    orders on EVERY case) are asked of the cases given; everything else of the whole list."""
    have = facts(cases)
    return [w for w in wanted(tuple(cases)) if w not in have]
