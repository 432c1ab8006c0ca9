"""The decode matvecs of the f32-activation weight types (F16, Q4_0, Q8_0 with GL3_FLAG_F32_ACTIVATION): the rule by which launch_matvec picks
a kernel, its workgroup, grid and LDS (vl_matvec_plan, csrc/gl3_veclane_kernels.h) restated in Python, and the grid of shapes that reaches
every form of it.

Every case is a Llama-architecture model of 1 layer with heads of 32 elements; n_heads * head_size (q_dim) need not be dim, so rows and K
of each projection move on their own:
    qkv      rows q_dim + 2 kv_dim, K dim      RMSNorm in front, store
    wo       rows dim,              K q_dim    residual
    gate/up  rows hidden,           K dim      RMSNorm in front, SwiGLU (two matrices)
    down     rows dim,              K hidden   residual
    logits   rows vocab,            K dim      RMSNorm in front, store
A case names the weight kinds (k_shapes.KINDS) it runs; a dimension may be a dict kind -> value where the legal step of the kind (64 F16 and
scalar order, 128 Q8_0, 256 vector-order Q4_0) moves the edge.

The rule:
    scalar order (f16s, q4s)     matvec_rl_kernel, 64 rows per workgroup of 9 wavefronts; rmsnorm_f32_kernel in front of an RMS launch
    vector order, RMS launch that is not residual, 1024 <= K <= 5120:  matvec_vl_kernel with the RMSNorm in its prologue, 4 groups of 8 rows
                                 per workgroup — for Q4_0 / Q8_0 only when groups x matrices > 512, else rmsnorm_f32_kernel + the K-split kernel
    vector order otherwise       F16: matvec_vl_kernel, 2 groups per workgroup; Q4_0 / Q8_0: matvec_vlq_kernel, one group per workgroup of
                                 nw wavefronts (vq_waves: 16 below 256 groups, 8 below 512, else 4 — 8 when K has more than 4 RCM chunks —
                                 halved down to 4 while nch < nw), MAXW 16 iff nw = 16, the partition of vq_partition
What the rule cannot reach, and the grid therefore does not ask for:
    * 255 and 511 groups: rows are dim or hidden (multiples of the kind's step) or the vocabulary (a multiple of 16), so "below" is the
      nearest legal row count under the threshold: 254 / 510 groups for the logits, threshold - step rows for wo / down and gate / up.
    * the promotion 4 -> 8 at exactly 4 RCM chunks and one more for SwiGLU: 4 RCM chunks are K = 4096 (Q4_0) or 3072 (Q8_0), inside
      vl_rms_fusable's range, where a gate/up launch of 512 or more groups takes the fused matvec_vl_kernel.  Asked for instead: K on the
      last legal step below 1024 (nw stays 4) and on the first above 5120 (promoted).
    * a group count that is no multiple of the workgroup's groups for matvec_vl_kernel without the prologue (2 groups per workgroup: every
      row count here is a multiple of 16), and rows that are no multiple of 64 for the residual and SwiGLU forms of matvec_rl_kernel (dim
      and hidden are multiples of 64).
tests/test_matvec_shapes.py holds the rule to the library's own answer (gl3_debug_matvec_plan) and asserts what the grid covers;
tests/test_gpu_matvec_shapes.py runs the grid against the oracle."""
import k_shapes as ks

KINDS = {k: ks.KINDS[k] for k in ("f16v256", "f16v512", "q4v256", "q8f32", "f16s", "q4s")}
KSPLIT, F16_VEC, SCALAR = ("q4v256", "q8f32"), ("f16v256", "f16v512"), ("f16s", "q4s")
CHUNK = {"q4v256": 256, "q8f32": 128, "f16v256": 64, "f16v512": 64}      # elements of one VL chunk
STEP = {"f16v256": 64, "f16v512": 64, "q4v256": 256, "q8f32": 128, "f16s": 64, "q4s": 64}
RL, VL_RMS, VL, VLQ = "matvec_rl_kernel", "matvec_vl_kernel<RMS>", "matvec_vl_kernel", "matvec_vlq_kernel"
VL_WAVES, VL_RMS_WAVES, RL_WAVES, RL_PITCH = 2, 4, 9, 68
FUSE_MIN_WAVES = 512               # a K-split type fuses the prologue only above this many groups x matrices
VL_LDS_CAP, RL_LDS_CAP = 64 * 1024, 160 * 1024 - 256
VQ_LDS_CAP = 2 * 64 * 4 + (16384 + 16 * 256) * 4      # matvec_vlq_kernel: gl3_create raises its limit (one chunk per wavefront beyond the largest K)
HEAD_SIZE, CTX = 32, 16
GRANITE = dict(embedding_scale=12.0, attention_scale=0.015625, residual_scale=0.22, logit_scale=8.0)      # tiny-granite's


# ---- the rule
def ceil_div(a, b):
    return (a + b - 1) // b


def round_chunks(kind, maxw, nm):
    """vq_round_chunks: chunks a wavefront holds per round (integer divisions in the header's order)"""
    return (8 if kind == "q4v256" else 12) // (2 if maxw == 16 else 1) // nm


def vq_waves(kind, k, nm, ngroups):
    nch, nw = k // CHUNK[kind], 4
    while nw < 16 and ngroups * nw < 2048:
        nw *= 2
    if nw == 4 and nch > 4 * round_chunks(kind, 8, nm):
        nw = 8
    while nw > 4 and nch < nw:
        nw //= 2
    return nw


def vq_partition(nch, nw, rcm):
    nrounds = ceil_div(nch, nw * rcm)
    return nrounds, ceil_div(nch, nw * nrounds)


def rms_fusable(k):
    return ks.SS_LO <= k <= ks.SS_HI and k % 4 == 0


def plan(kind, pro, epi, rows, k):
    """What gl3_debug_matvec_plan answers.  pro: "rms" | "quant"; epi: "store" | "resid" | "swiglu" """
    nm, ngroups = 2 if epi == "swiglu" else 1, ceil_div(rows, 8)
    vector = kind not in SCALAR
    fuse = pro == "rms" and vector and rms_fusable(k) and epi != "resid" and not (kind in KSPLIT and ngroups * nm <= FUSE_MIN_WAVES)
    p = dict(kernel=None, rms_launch=int(pro == "rms" and not fuse), nw=0, MAXW=0, grid=0, threads=0, lds=0, lds_cap=VL_LDS_CAP, nch=0, nrounds=0, rc=0, RCM=0)
    if not vector:
        p.update(kernel=RL, nw=RL_WAVES, grid=ceil_div(rows, 64), lds=(k + 2 * nm * 64 * RL_PITCH) * 4, lds_cap=RL_LDS_CAP)
    elif fuse:
        p.update(kernel=VL_RMS, nw=VL_RMS_WAVES, grid=ceil_div(ngroups, VL_RMS_WAVES), lds=k * 4 + (k + 32) * 4 + ks.ss_scratch_bytes(k) + 16)
    elif kind in F16_VEC:
        p.update(kernel=VL, nw=VL_WAVES, grid=ceil_div(ngroups, VL_WAVES), lds=k * 4)
    else:
        nw = vq_waves(kind, k, nm, ngroups)
        maxw = 16 if nw == 16 else 8
        nch, rcm = k // CHUNK[kind], round_chunks(kind, maxw, nm)
        nrounds, rc = vq_partition(nch, nw, rcm)
        p.update(kernel=VLQ, nw=nw, MAXW=maxw, grid=ngroups, lds_cap=VQ_LDS_CAP, lds=nm * 64 * 4 + nw * rc * CHUNK[kind] * 4, nch=nch, nrounds=nrounds, rc=rc, RCM=rcm)
    p["threads"] = 64 * p["nw"]
    return p


def slots(pl):
    """matvec_vlq_kernel: (round, wavefront, first chunk, chunks) in chain order — c_lo = (r nw + w) rc, nc = max(0, min(rc, nch - c_lo))"""
    return [(r, w, (r * pl["nw"] + w) * pl["rc"], max(0, min(pl["rc"], pl["nch"] - (r * pl["nw"] + w) * pl["rc"])))
            for r in range(pl["nrounds"]) for w in range(pl["nw"])]


def issue_reads(kind, pl, r, w, xq):
    """What VQ_ISSUE(r) of wavefront w loads, clamped as the kernel clamps: (first chunk c_lo_, chunks nc_, the chunk index of every weight
    load u < RCM, the float4 index into x of every activation load (u, lane) — in floats / 4 from the start of x)"""
    ce, nch, rc = CHUNK[kind], pl["nch"], pl["rc"]
    c_lo = min((r * pl["nw"] + w) * rc, nch - 1)
    nc = max(1, min(rc, nch - c_lo))
    nq = nc * (ce // 4)
    chunks = [c_lo + min(u, nc - 1) for u in range(pl["RCM"])]
    quads = [c_lo * (ce // 4) + min(u * 64 + lane, nq - 1) for u in range(xq) for lane in range(64)]
    return c_lo, nc, chunks, quads


def x_quads(kind, rcm):
    """XQ of matvec_vlq_kernel: float4 loads per lane that stage a round's slice, rounded up"""
    return (rcm * CHUNK[kind] + 255) // 256


# ---- the cases.  kinds: which weight kinds run the case; a dimension that depends on the kind is a dict
def _per(q4, q8):
    return {"q4v256": q4, "q8f32": q8}


CASES = {
    # A: 512 groups of wo / down at one or two chunks: nw 4 with idle wavefronts (nch 1: Q4_0 K 256; nch 2: Q8_0), halving has nothing to do
    # at 4; logits at 512 groups keep the separate RMSNorm (512 wavefronts, not more) although dim is inside the fusable range
    "A": dict(dim=4096, q_dim=256, hidden=256, vocab=4096, kinds=KSPLIT),
    # the same one step of dim lower: wo / down below 512 groups start at nw 8 and halve to 4; logits at 510 groups: nw 8
    "A-below": dict(dim=_per(3840, 3968), q_dim=256, hidden=256, vocab=4080, kinds=KSPLIT),
    # B: down promoted 4 -> 8 one chunk above 4 RCM (Q4_0 nch 33: rc 5, last 3, one idle; Q8_0 nch 49: rc 7); gate/up fused (1056 groups);
    # logits 514 groups: fused, 2 of 4 groups in the last workgroup
    "B": dict(dim=4096, q_dim=256, hidden=_per(8448, 6272), vocab=4112, kinds=KSPLIT),
    # (its down of Q4_0 is also the candidate "wo at nw 8 with 9 chunks: rc 2, a last wavefront of 1, three idle" — G-above's down has it)
    # ... and at exactly 4 RCM chunks: nw stays 4, rc = RCM, every register slot of every wavefront full
    "B-at": dict(dim=4096, q_dim=256, hidden=_per(8192, 6144), vocab=96, kinds=KSPLIT),
    # C: nw 8 / MAXW 8 at K 12544: Q4_0 49 chunks, rc 7, uniform; Q8_0 98 chunks in two rounds of rc 7, the second with two idle slots
    "C": dict(dim=2048, q_dim=256, hidden=12544, vocab=2048, kinds=KSPLIT),
    # the same one step of dim lower (below 256 groups: nw 16); logits at 254 groups
    "C-below": dict(dim=_per(1792, 1920), q_dim=256, hidden=256, vocab=2032, kinds=KSPLIT),
    # D: nw 16 / MAXW 16 at K 12544: Q4_0 rc 4 with a last wavefront of 1; Q8_0 two rounds
    "D": dict(dim=256, q_dim=256, hidden=12544, vocab=96, kinds=KSPLIT, granite=True),
    # E: non-fused gate/up (K above 5120) at nw 16: two rounds, the second ragged (Q4_0 33 chunks: 32 + 1; Q8_0 50 chunks: 32 + 18)
    "E": dict(dim=_per(8448, 6400), q_dim=256, hidden=256, vocab=96, kinds=KSPLIT),
    # two rounds at MAXW 8 for Q4_0: only with two matrices (RCM 4: 33 chunks = 24 + 9, the second round ragged); one matrix would need
    # 65 chunks, K = 16640, above the 16384 the vector order accepts
    "E8": dict(dim=8448, q_dim=256, hidden=2048, vocab=96, kinds=("q4v256",)),
    # gate/up at 256 groups (512 wavefronts: separate RMSNorm inside the fusable range, nw 8) and one step of hidden above (fused)
    "G-at": dict(dim=1024, q_dim=256, hidden=2048, vocab=96, kinds=KSPLIT),
    "G-above": dict(dim=1024, q_dim=256, hidden=_per(2304, 2176), vocab=96, kinds=KSPLIT),
    # gate/up below 256 groups at a K below the fusable range: nw 16 halved by nch (Q4_0 3 chunks -> 4; Q8_0 7 chunks -> 4)
    "G-below": dict(dim=_per(768, 896), q_dim=256, hidden=_per(1792, 1920), vocab=96, kinds=KSPLIT),
    # gate/up around 512 groups outside the fusable range: one step of hidden below 512 groups at K on the last step below 1024 (nw 8 halved
    # to 4), and 512 groups at K on the first step above 5120 (promoted to 8; D has the unpromoted nw 4 at K 256)
    "S-low-below": dict(dim=_per(768, 896), q_dim=256, hidden=_per(3840, 3968), vocab=96, kinds=KSPLIT),
    "S-high": dict(dim=_per(5376, 5248), q_dim=256, hidden=4096, vocab=96, kinds=KSPLIT),
    # halving from 16 to 8 (8 <= nch < 16) and nch 1 for Q8_0 (q_dim 128)
    "H": dict(dim=256, q_dim=_per(256, 128), hidden=_per(3072, 1536), vocab=96, kinds=KSPLIT),
    # matvec_vl_kernel of F16 at both species: inside the fusable range (logits 130 groups: 2 of 4 in the last workgroup; gate/up 32: full),
    # below and above it (2 groups per workgroup)
    "V-in": dict(dim=1024, q_dim=256, hidden=256, vocab=1040, kinds=F16_VEC),
    "V-below": dict(dim=960, q_dim=256, hidden=256, vocab=96, kinds=F16_VEC),
    "V-above": dict(dim=5184, q_dim=256, hidden=256, vocab=96, kinds=F16_VEC),
    # matvec_rl_kernel: logits of 96 rows (a workgroup of 32 rows behind a full one), qkv of 384 (full), residual and SwiGLU
    "R": dict(dim=256, q_dim=256, hidden=320, vocab=96, kinds=SCALAR),
}
EAGER = ["B", "C", "D", "E", "E8"]          # the cases that own the ragged and multi-round facts run once more with FLAG_NO_GRAPH
EDGE = ["B", "D"]                          # ... and these carry the edge-value edits, for Q4_0 and for F16
GRID = [(c, k) for c in CASES for k in CASES[c]["kinds"]]


def dims(case, kind):
    c = CASES[case]
    d = {f: (c[f][kind] if isinstance(c[f], dict) else c[f]) for f in ("dim", "q_dim", "hidden", "vocab")}
    assert all(d[f] % STEP[kind] == 0 for f in ("dim", "q_dim", "hidden")) and d["vocab"] % 16 == 0, (case, kind, d)
    d["heads"] = d["q_dim"] // HEAD_SIZE
    d["kv_heads"] = max(1, d["heads"] // 4)
    return d


def case_config(synth, case, kind):
    d = dims(case, kind)
    granite = CASES[case].get("granite")
    return synth.ModelConfig("mv-%s-%s" % (case, kind), synth.ARCH_GRANITE if granite else synth.ARCH_LLAMA, d["dim"], d["hidden"], 1, d["heads"],
                             d["kv_heads"], HEAD_SIZE, d["vocab"], CTX, 1e-5, 500000.0, False, **(GRANITE if granite else {}))


def case_model(pkg, case, kind, seed=47):
    return pkg.synth.make_numpy(case_config(pkg.synth, case, kind), wtype=KINDS[kind]["wtype"], seed=seed)


def kind_flags(hip, kind):
    f = 0
    for n in KINDS[kind]["flags"]:
        f |= getattr(hip, n)
    return f


def launches(case, kind):
    """The matvec launches of a decode step of the case: (projection, pro, epi, rows, K, out_scale != 1)"""
    d, scaled = dims(case, kind), bool(CASES[case].get("granite"))
    return [("qkv", "rms", "store", d["q_dim"] + 2 * d["kv_heads"] * HEAD_SIZE, d["dim"], False), ("wo", "quant", "resid", d["dim"], d["q_dim"], scaled),
            ("gate/up", "rms", "swiglu", d["hidden"], d["dim"], False), ("down", "quant", "resid", d["dim"], d["hidden"], scaled),
            ("logits", "rms", "store", d["vocab"], d["dim"], scaled)]


# ---- what a launch reaches
def nearest_below(kind, proj, groups):
    """the largest group count under `groups` that the projection's rows can take: vocab moves in 16 rows, dim and hidden in the kind's step"""
    return groups - (2 if proj == "logits" else STEP[kind] // 8)


def k_side(k):
    return "K below 1024" if k < ks.SS_LO else "K above 5120" if k > ks.SS_HI else "K fusable"


def launch_facts(kind, proj, pro, epi, rows, k, scaled):
    pl, ngroups, nm = plan(kind, pro, epi, rows, k), ceil_div(rows, 8), 2 if epi == "swiglu" else 1
    have = set()
    if pl["kernel"] == RL:
        have.add(("rl", kind, epi, "full" if rows % 64 == 0 else "row tail"))
        return have
    if pl["kernel"] in (VL, VL_RMS):
        rest = ngroups % pl["nw"]
        have.add((pl["kernel"], kind, epi, "full" if rest == 0 else "%d of %d groups" % (rest, pl["nw"])))
        if kind in F16_VEC and pro == "rms":
            have.add(("rms", kind, k_side(k)))
        if kind in KSPLIT and ngroups * nm <= FUSE_MIN_WAVES + 2 * STEP[kind] // 8:
            have.add(("512 wavefronts", kind, epi, "above"))
        return have
    nw, nch, rc, rcm = pl["nw"], pl["nch"], pl["rc"], pl["RCM"]
    have |= {("nw", kind, epi, nw), ("epi", kind, epi)}
    if pro == "rms":                                         # why a store / SwiGLU launch is here and not on the fused kernel
        have.add(("non-fused", kind, epi, k_side(k) if not rms_fusable(k) else "at most 512 wavefronts"))
        if rms_fusable(k) and ngroups * nm == FUSE_MIN_WAVES:
            have.add(("512 wavefronts", kind, epi, "at"))
    for edge in (256, 512):
        if ngroups == edge:
            have.add(("groups", kind, epi, edge, "at"))
        if ngroups == nearest_below(kind, proj, edge):
            have.add(("groups", kind, epi, edge, "below"))
    if ngroups >= 512:
        if epi != "swiglu" and nch in (4 * rcm, 4 * rcm + 1):
            have.add(("promotion", kind, epi, "4 RCM chunks" if nch == 4 * rcm else "one chunk more"))
        if epi == "swiglu" and not rms_fusable(k):
            have.add(("promotion", kind, epi, "promoted" if nw == 8 else "not promoted"))
    start = 4 if ngroups >= 512 else 8 if ngroups >= 256 else 16
    if nw < start:
        have.add(("halved", kind, start, nw))
    if nw == 4 and nch < 4:
        have.add(("nch < 4 at nw 4", kind))
    if nch == 1:
        have.add(("nch 1", kind))
    sl = slots(pl)
    ncs = [nc for _, _, _, nc in sl]
    if all(nc == rc for nc in ncs):
        have.add(("uniform", kind))
    if any(0 < nc < rc for nc in ncs):
        have.add(("last wavefront short", kind))
    if any(nc == 0 for nc in ncs):
        have.add(("idle wavefronts", kind))
    if pl["nrounds"] >= 2:
        have.add(("rounds >= 2", kind, pl["MAXW"]))
        if all(nc == rc for nc in ncs[:nw]) and any(nc < rc for nc in ncs[-nw:]):
            have.add(("ragged last round", kind))
        if epi == "swiglu":
            have.add(("rounds >= 2 with two matrices", kind))
    if rc == rcm:
        have.add(("rc == RCM", kind))
    if rc == 1:
        have.add(("rc == 1", kind))
    if scaled:
        have.add(("out_scale", epi))
    return have


def facts(cases):
    have = set()
    for case in cases:
        for kind in CASES[case]["kinds"]:
            for l in launches(case, kind):
                have |= launch_facts(kind, *l)
    return have


def wanted():
    req = []
    for kind in KSPLIT:
        req += [("nw", kind, epi, nw) for epi in ("resid", "store", "swiglu") for nw in (4, 8, 16)]
        req += [("groups", kind, epi, edge, side) for epi in ("resid", "store", "swiglu") for edge in (256, 512) for side in ("below", "at")]
        req += [("promotion", kind, "resid", "4 RCM chunks"), ("promotion", kind, "resid", "one chunk more"),
                ("promotion", kind, "swiglu", "not promoted"), ("promotion", kind, "swiglu", "promoted")]
        req += [("halved", kind, 16, 8), ("halved", kind, 16, 4), ("halved", kind, 8, 4), ("nch < 4 at nw 4", kind), ("nch 1", kind)]
        req += [("uniform", kind), ("last wavefront short", kind), ("idle wavefronts", kind), ("rounds >= 2", kind, 8), ("rounds >= 2", kind, 16),
                ("ragged last round", kind), ("rounds >= 2 with two matrices", kind), ("rc == RCM", kind), ("rc == 1", kind)]
        req += [("epi", kind, epi) for epi in ("resid", "store", "swiglu")]
        req += [("non-fused", kind, epi, why) for epi in ("store", "swiglu") for why in ("K below 1024", "K above 5120", "at most 512 wavefronts")]
        req += [("512 wavefronts", kind, epi, side) for epi in ("store", "swiglu") for side in ("at", "above")]
        req += [(VL_RMS, kind, "store", "2 of 4 groups"), (VL_RMS, kind, "swiglu", "full")]
    req += [("out_scale", "resid"), ("out_scale", "store")]
    for kind in F16_VEC:
        req += [(VL_RMS, kind, "store", "2 of 4 groups"), (VL_RMS, kind, "store", "full"), (VL_RMS, kind, "swiglu", "full"),
                (VL, kind, "resid", "full"), (VL, kind, "store", "full"), (VL, kind, "swiglu", "full"),
                ("rms", kind, "K below 1024"), ("rms", kind, "K fusable"), ("rms", kind, "K above 5120")]
    for kind in SCALAR:
        req += [("rl", kind, "store", "full"), ("rl", kind, "store", "row tail"), ("rl", kind, "resid", "full"), ("rl", kind, "swiglu", "full")]
    return req


def missing(cases):
    """Requirements that the cases `cases` do not meet (empty: the grid covers everything)"""
    have = facts(cases)
    return [w for w in wanted() if w not in have]


def unneeded(cases):
    """Cases without which the rest covers the same requirements (empty: every case brings a fact no other case brings)"""
    return [c for c in cases if not missing([x for x in cases if x != c])]
