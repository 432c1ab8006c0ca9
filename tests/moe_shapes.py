"""The Qwen2-MoE configuration grid: the expert counts, top-k, expert sizes and shared-expert sizes at which the routing kernels, the
merged shared slots of the decode launch, the expert projections and the batched grouping take another branch, and the rule that says
which branch a case takes.

Every case is tiny-qwen2moe (dim 256, 2 layers, 8 query heads on 2 kv heads of 32, vocab 512) with ctx 96 and only n_experts,
n_experts_used, moe_hidden and hidden (the shared expert's size) overridden.

The rule below restates, in Python, conditions of gl3_moe_kernels.h (moe_router_token, moe_router_wgs, moe_group_kernel,
moe_group_max_entries, moe_combine_kernel), gl3_decode_kernels.h (seq_sum_lds, the SEL prologue of matvec_q8t_kernel) and gl3_api.hip
(launch_matvec_sel, gl3_create).  tests/test_moe_shapes.py asserts what the grid covers, that every row is needed for it, that the constants
are the ones in the kernel sources and that both oracles agree at these shapes; tests/test_gpu_moe_shapes.py runs the grid."""

MOE_RR = 8                      # moe_router_token: router rows per workgroup
WAVE = 64                       # the softmax / top-k wavefront of the router's last workgroup; moe_group_kernel's ballot width
SUM_PIPELINE_MIN = 16           # seq_sum_lds: the software pipeline serves n >= 16, shorter sums go straight to the quad / scalar loops
MOE_GROUP_THREADS = 1024        # moe_group_kernel: 16 wavefronts, wavefront w owns experts w, w + 16, ...
TOPK_MAX, EXPERTS_MAX = 64, 4096        # gl3_create; the C oracle keeps moe_sel[64]
DIM, LAYERS, HEADS, KV_HEADS, HEAD_SIZE, VOCAB, CTX = 256, 2, 8, 2, 32, 512, 96
SHORT, LONG = 17, 65            # the two chunks of the batched test: past the 16-token tile, on the > 64-token path
DECODE_STEPS = 4                # single-token decode steps at positions 0 .. 3, on the first tokens of the long chunk

#  name -> (n_experts, n_experts_used, moe_hidden, shared hidden, model seed).  The seed is picked on the CPU so that the oracle's own routing
#  meets the claims of the case (claims() below); tests/test_moe_shapes.py asserts that it does.
GRID = {
    "e1-k1":       (1, 1, 128, 512, 41),
    "e7-k7":       (7, 7, 96, 320, 41),
    "e8-k2-sh64":  (8, 2, 128, 64, 41),
    "e8-k2-sh128": (8, 2, 128, 128, 41),
    "e63-k3":      (63, 3, 32, 512, 41),
    "e64-k8":      (64, 8, 160, 1280, 41),
    "e65-k4":      (65, 4, 128, 512, 55),
    "e64-k64":     (64, 64, 32, 96, 41),
    "e130-k6":     (130, 6, 64, 160, 43),
}


# ---- the rule
def moe_router_wgs(experts):
    """workgroups of a token's router launch: n_experts rows and the shared-gate row, MOE_RR to a workgroup"""
    return (experts + 1 + MOE_RR - 1) // MOE_RR


def router_padding_rows(experts):
    """rows of the last workgroup past the shared-gate row: they alias it and store nothing"""
    return moe_router_wgs(experts) * MOE_RR - (experts + 1)


def gate_row_place(experts):
    """where the shared-gate row sits in its workgroup"""
    at = experts % MOE_RR
    return "alone" if at == 0 else "closes a full workgroup" if at == MOE_RR - 1 else "inside"


def scan_trips(experts):
    """trips of `for (i = t; i < E; i += 64)` in the softmax and in every top-k round"""
    return (experts + WAVE - 1) // WAVE


def softmax_sum_form(experts):
    """seq_sum_lds<false>(e, E) -> (form, quads behind the pipeline, scalar tail elements)"""
    if experts < SUM_PIPELINE_MIN:
        return "short", experts // 4, experts % 4
    piped = experts // 8 * 8
    return "pipelined", (experts - piped) // 4, experts % 4


def shared_slots(hidden, moe_hidden):
    """the shared expert's gate / up rows as extra blockIdx.y slots of the routed experts' decode launch -> (slots, rows of the last slot if it
    is cut short, else 0)"""
    slots = (hidden + moe_hidden - 1) // moe_hidden
    left = hidden - (slots - 1) * moe_hidden
    return slots, left if left < moe_hidden else 0


def shared_slot_rows(hidden, moe_hidden):
    slots, tail = shared_slots(hidden, moe_hidden)
    return [moe_hidden] * (slots - 1) + [tail or moe_hidden]


def k_blocks(k):
    """Q8_0 blocks of an inner dimension and the zero blocks that pad its last 4-block tile group"""
    blocks = k // 32
    return blocks, -blocks % 4


def moe_group_max_entries(n, topk, experts):
    s = n * topk
    return min(experts, s) + s // 16


def experts_per_group_wave(experts):
    """the most experts one wavefront of moe_group_kernel owns"""
    waves = MOE_GROUP_THREADS // WAVE
    return (experts + waves - 1) // waves


def combine_terms(topk):
    """moe_combine_kernel: the selected experts, then the shared expert"""
    return topk + 1


def facts(name):
    """Every branch quantity of a case, as the requirement list below reads them"""
    experts, topk, mh, hidden, _ = GRID[name]
    form, quads, tail = softmax_sum_form(experts)
    slots, slot_tail = shared_slots(hidden, mh)
    return dict(experts=experts, topk=topk, moe_hidden=mh, hidden=hidden, wgs=moe_router_wgs(experts), padding=router_padding_rows(experts),
                gate_row=gate_row_place(experts), trips=scan_trips(experts), sum_form=form, sum_quads=quads, sum_tail=tail, slots=slots,
                slot_tail=slot_tail, expert_blocks=k_blocks(mh), shared_blocks=k_blocks(hidden), wave_experts=experts_per_group_wave(experts),
                terms=combine_terms(topk), rows_long=LONG * topk, entries_long=moe_group_max_entries(LONG, topk, experts))


#  what the grid must hold: (requirement, predicate over a case's facts)
WANTED = [
    ("router: the gate row closes a full workgroup (E % 8 == 7), one workgroup", lambda f: f["gate_row"] == "closes a full workgroup" and f["wgs"] == 1),
    ("router: the gate row closes a full workgroup, several workgroups", lambda f: f["gate_row"] == "closes a full workgroup" and f["wgs"] > 1),
    ("router: the gate row alone in its workgroup (E % 8 == 0), 7 padding rows", lambda f: f["gate_row"] == "alone" and f["padding"] == 7),
    ("router: E = 64 with top-8, Qwen2-57B-A14B's routing shape", lambda f: (f["experts"], f["topk"]) == (64, 8)),
    ("router: one expert", lambda f: f["experts"] == 1),
    ("scan: E equals the wavefront width, one trip", lambda f: f["experts"] == WAVE),
    ("scan: E = 65, index 64 on the second trip", lambda f: f["experts"] == WAVE + 1),
    ("scan: three trips", lambda f: f["trips"] == 3),
    ("softmax sum: short form with a scalar tail", lambda f: f["sum_form"] == "short" and f["sum_tail"] > 0 and f["sum_quads"] > 0),
    ("softmax sum: short form, whole quads", lambda f: f["sum_form"] == "short" and f["sum_tail"] == 0 and f["sum_quads"] > 0),
    ("softmax sum: short form, fewer than four elements", lambda f: f["sum_form"] == "short" and f["sum_quads"] == 0),
    ("softmax sum: pipelined with a quad and a scalar tail", lambda f: f["sum_form"] == "pipelined" and f["sum_quads"] > 0 and f["sum_tail"] > 0),
    ("softmax sum: pipelined with a scalar tail alone", lambda f: f["sum_form"] == "pipelined" and f["sum_quads"] == 0 and f["sum_tail"] > 0),
    ("softmax sum: pipelined, no tail", lambda f: f["sum_form"] == "pipelined" and f["sum_quads"] == 0 and f["sum_tail"] == 0),
    ("top-k: 1", lambda f: f["topk"] == 1),
    ("top-k: every expert, more than one", lambda f: f["topk"] == f["experts"] > 1),
    ("top-k: the limit of 64", lambda f: f["topk"] == TOPK_MAX),
    ("shared slots: smaller than one expert, the tail on the first slot", lambda f: f["slots"] == 1 and f["slot_tail"] > 0),
    ("shared slots: exactly one whole slot", lambda f: f["slots"] == 1 and f["slot_tail"] == 0),
    ("shared slots: several with a tail on the last", lambda f: f["slots"] > 2 and f["slot_tail"] > 0),
    ("shared slots: 64 selected slots and three shared ones", lambda f: f["slots"] == 3 and f["topk"] == TOPK_MAX),
    ("shared slots: two whole ones and a tail at expert K = 64", lambda f: f["slots"] == 3 and f["slot_tail"] > 0 and f["moe_hidden"] == 64),
    ("expert K: one block, three padded", lambda f: f["expert_blocks"] == (1, 3)),
    ("expert K: two blocks, two padded", lambda f: f["expert_blocks"] == (2, 2)),
    ("expert K: three blocks, one padded", lambda f: f["expert_blocks"] == (3, 1)),
    ("expert K: five blocks, the second tile group padded", lambda f: f["expert_blocks"] == (5, 3)),
    ("shared K: below 256 with a padded tile group (2 blocks)", lambda f: f["shared_blocks"] == (2, 2)),
    ("shared K: below 256 with a padded tile group (3 blocks)", lambda f: f["shared_blocks"] == (3, 1)),
    ("shared K: below 256 with a padded tile group (5 blocks)", lambda f: f["shared_blocks"] == (5, 3)),
    ("shared K: exactly one tile group", lambda f: f["shared_blocks"] == (4, 0)),
    ("shared K: ten blocks, not a multiple of the expert size", lambda f: f["shared_blocks"] == (10, 2)),
    ("grouping: a wavefront owns several experts", lambda f: f["wave_experts"] >= 9),
    ("grouping: a wavefront owns five experts, one of them beyond the first trip's width", lambda f: f["wave_experts"] == 5),
    ("batched: S = 64 n rows of the routed operand and a 65-term combine", lambda f: f["rows_long"] == 64 * LONG and f["terms"] == 65),
    ("batched: fewer assignments than experts at 17 tokens", lambda f: SHORT * f["topk"] < f["experts"]),
]


def missing(names):
    """Requirements that the cases `names` do not meet (empty: the grid covers everything)"""
    fs = [facts(n) for n in names]
    return [what for what, ok in WANTED if not any(ok(f) for f in fs)]


def case_config(synth, name):
    experts, topk, mh, hidden, _ = GRID[name]
    b = synth.CONFIGS["tiny-qwen2moe"]
    assert (b.dim, b.n_layers, b.n_heads, b.n_kv_heads, b.head_size, b.vocab) == (DIM, LAYERS, HEADS, KV_HEADS, HEAD_SIZE, VOCAB)
    return synth.ModelConfig(**{**b.__dict__, "name": "moe-" + name, "ctx": CTX, "n_experts": experts, "n_experts_used": topk, "moe_hidden": mh,
                                "hidden": hidden})


def case_model(pkg, name, seed=None):
    return pkg.synth.make_numpy(case_config(pkg.synth, name), wtype=8, seed=GRID[name][4] if seed is None else seed)


def decode_tokens(pkg):
    return pkg.javarand.bench_tokens(VOCAB, DECODE_STEPS)


def chunk_tokens(pkg):
    """(the 17-token chunk of sequence 0, the 65-token chunk of sequence 1 and the token behind it)"""
    long_ = pkg.javarand.bench_tokens(VOCAB, LONG + 1)
    assert long_[:DECODE_STEPS] == decode_tokens(pkg)
    return pkg.javarand.bench_tokens(VOCAB, SHORT + 7)[7:], long_


# ---- what a case has to prove about itself, from the oracle's routing alone
def claims(name, short_sel, long_sel):
    """short_sel / long_sel: the oracle's expert ids [rows][topk] of the last layer for the 17- and the 65-token chunk.  Returns the claims of
    the case that do NOT hold (empty: the case is the case it says it is)."""
    experts, topk = GRID[name][:2]
    rows = [list(r) for r in short_sel] + [list(r) for r in long_sel]
    assert len(short_sel) == SHORT and len(long_sel) == LONG and all(len(r) == topk for r in rows)
    count = lambda sel: [sum(list(r).count(e) for r in sel) for e in range(experts)]
    bad = []
    if any(len(set(r)) != topk or min(r) < 0 or max(r) >= experts for r in rows):
        bad.append("a row's selection is not %d distinct experts" % topk)
    if topk == experts and any(sorted(r) != list(range(experts)) for r in rows):
        bad.append("top-k = E: a row's selection is not a permutation of all experts")
    # the single-token decode steps run the first DECODE_STEPS tokens of the long chunk at the same positions: the claim holds there too
    decode = [list(r) for r in long_sel[:DECODE_STEPS]]
    if name == "e65-k4" and not (any(64 in r for r in rows) and any(64 in r for r in decode)):
        bad.append("no row selects expert 64")
    if name == "e130-k6" and not (any(max(r) >= 128 for r in rows) and any(max(r) >= 128 for r in decode)):
        bad.append("no row selects an expert >= 128")
    if name == "e130-k6" and sum(1 for c in count(short_sel) if c == 0) < 28:
        bad.append("fewer than 28 experts stay empty at 17 tokens")
    if name == "e64-k64" and any((c + 15) // 16 != 5 for c in count(long_sel)):
        bad.append("an expert does not own 5 table entries in the 65-token chunk")
    if name in ("e63-k3", "e64-k8") and max(count(long_sel)) <= 16:
        bad.append("no expert holds more than 16 assignments at 65 tokens")
    return bad
