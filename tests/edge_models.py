"""TEST HELPER — synthetic models whose VALUES sit on the edges the random N(0, 0.02^2) models never reach.

make_edge_model(cfg_name, wtype, seed, edits, **cfg_overrides) takes synth.make_numpy(...) and rewrites raw tensor bytes; the result
is still a SynthModel, so HipMasterPlan, COracle, NpOracle and write_gguf take it unchanged.  Every edit has a name (EDITS); "all"
applies the whole set.  Everything is a pure function of (config, type, seed, edits).  NaN and +-Inf never appear.

Layout of the edits on a model of nb = dim / 32 activation blocks (the tiny configs: 8, ragged-llama: 9):
  act-blocks        norm gains per 32-channel block (multiplied onto the 1 + N(0, 0.02^2) gain)
                       attn_norm    block 1: 0     block 2: ROUND0   block 3: SUBN     block nb-1: OUTLIER
                       ffn_norm     block 0: OUTLIER   block 1: ROUND0   block nb-2: 0   block nb-1: SUBN
                       output_norm  block 0: ROUND0    block 1: SUBN     block 2: OUTLIER   block nb-1: 0
                    ROUND0 = 1e-7: |xhat| <= sqrt(dim) <= 17, so amax / 127 < 2^-25 and the f16 activation scale is 0 while the int8
                    values (computed from the f32 scale) are not; SUBN = 2e-4: scale f16-subnormal while 0.04 < block amax of xhat < 38;
                    OUTLIER = 3e3.  Token ZERO_TOKEN's embedding row dequantises to exactly zero (every d = 0 / every f16 = +0).
                    Qwen3: attn_q_norm / attn_k_norm element 5 = 0, element 9 large (QN_LARGE / KN_LARGE: scores of a few tens).
  inner-act-blocks  attn_v rows 0..31 zero (qwen2 family: their bias too): the heads on them hand wo an all-zero block; with four or more
                    32-row groups, groups 1 and 2 shrunk by 2^-10 / 2^-19.  ffn_up (Phi-3: the up half; MoE: expert MOE_EXPERT and the
                    shared expert): group 1 zero, the following groups a ladder (UP_LADDER) that shrinks the up rows and, on the deep rungs,
                    the gate rows too — hb differs by 10^6 between the edit alone and "all"; one rung lands its block scale in the f16
                    subnormals in either.  Applied AFTER the weight edits, so that its zero rows stay zero.
  w-scales          (Q8_0 / Q4_0) in every matrix: d = 0 at (row 0, first block) and (last row, last block); d = 0x0001 at (row 0, last
                    block); 0x03FF at (row 1, first); 0x0400 at (row 1, last); Q8_0: sign of d flipped at (last row, first block) and in
                    all of row 7; d = 2^15 (v, gate, up and the expert stacks: 2^8 — with 2^15 the activation they
                    feed exceeds 65504 * 127 and ITS f16 scale is infinite) at (middle row + 9, quiet block) — the quiet block is the K block fed by the SUBN / shrunk
                    activation block, so the product stays of ordinary size when the activation edits are present.
  w-quants          Q8_0: all -128 at (row 2, first), all +127 at (row 2, last), alternating +-127 at (row 3, middle).  Token
                    FLAT_TOKEN's embedding has |q| = 127 with alternating signs in block nb-1 and layer 0's attn_norm is flat on that block
                    (the OUTLIER block), so its int8 activation block there is +-127 throughout; in attn_q of layer 0, row 4 matches the
                    signs (isum = 32 * 127 * 127 = 516128, the bound), row 5 is all -128 (the pairs cancel: isum = 0), row 6 holds -128
                    against +127 and +127 against -127 (isum = -16 * 127 * 255 = -518160).  Q4_0: nibbles all 0 at (row 2, first), all
                    15 at (row 2, last).
  f16-values        (F16) whole 16- and 8-element lane groups of subnormals, +-0, 0x7BFF and 0x0400 in the first / last rows and the
                    first / last K group, and the same values as single elements.
  peaked-attn       per-head edits of attn_q (and the K rows under those heads), see peaked_attn(): head 4 far out (terms exactly 0), head 5
                    at score gaps of ~10^2 (f32-subnormal terms), head 6 flat, the rest untouched.  A tie at the maximum comes from
                    ZERO_TOKEN used as the query (act-blocks): q = 0, every score is +-0.
  (sink head)       with act-blocks + inner-act-blocks + peaked-attn on Q8_0 llama / granite / qwen2moe: sink_head() scales head SINK_HEAD's
                    attn_q so that at position 1, behind ZERO_TOKEN, it hands wo a block with an f16-subnormal scale in every layer.
  moe-router        router row 2 = row 1 (exact tie), both x 4; row MOE_EXPERT x 1000: that expert is first for every token whose logit
                    on it is positive (routed_tokens() picks such tokens); every other probability is then exactly 0, a seven-way tie for
                    the second place that the lowest index wins.  Tokens whose logit on it is negative choose among the rest, rows 1 / 2
                    often both.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

F32 = np.float32
EDITS = ("act-blocks", "inner-act-blocks", "w-scales", "w-quants", "f16-values", "peaked-attn", "moe-router")
ZERO_TOKEN, FLAT_TOKEN = 3, 6
ROUND0, SUBN, OUTLIER = 1e-7, 2e-4, 3e3
QN_LARGE, KN_LARGE = 48.0, 6.0
MOE_EXPERT = 5
SINK_HEAD, SINK_TARGET = 7, 2.4e-4          # sink_head(): the head and the block amax it hands wo (middle of the f16-subnormal scale window * 127)
PEAK_SHIFT = {4: 3, 5: 0, 6: 0}                # head -> power of two on its attn_q rows, beside act-blocks
PEAK_SHIFT_ALONE = {4: 13, 5: 10, 6: -3}       # on the plain model (scores ~ 10^-1)
Q8, Q4, F16T = 8, 2, 1
# (power of two on the ffn_up rows, on the ffn_gate rows) of the 32-row groups 2, 3, ..: a Q8_0 row cannot shrink below about 2^-20 (one f16
# ulp of scale times a quant of 1), so the deep rungs shrink the gate rows as well (silu(g) ~ g / 2 for small g)
UP_LADDER = ((-10, 0), (-18, 0), (-18, -12), (-19, -16))
UP_LADDER_NARROW = ((-10, 0), (-18, -12))


def edits_for(wtype, arch, which):
    """The edits of `which` ("all", a name or a tuple of names) that exist for this weight type / architecture."""
    names = EDITS if which == "all" else (which,) if isinstance(which, str) else tuple(which)
    assert all(n in EDITS for n in names), names
    ok = []
    for n in names:
        if n in ("w-scales", "w-quants") and wtype not in (Q8, Q4):
            continue
        if n == "f16-values" and wtype != F16T:
            continue
        if n == "moe-router" and arch != 5:
            continue
        ok.append(n)
    return tuple(ok)


class Mat:
    """Rows [r0, r0 + rows) of a matrix tensor as editable blocks (Q8_0 / Q4_0) or f16 bit patterns."""

    def __init__(self, m, name, r0=0, rows=None):
        raw, ty, nrows, cols = m.tensors[name]
        assert raw.flags.writeable
        self.ty, self.cols, self.nb = ty, cols, cols // 32
        rows = nrows - r0 if rows is None else rows
        self.rows = rows
        self.big, self.big_row = 0x7800, rows // 2 + 9        # w-scales: the large block scale (2^15) and its row
        if ty == F16T:
            self.h = raw.view(np.uint16).reshape(nrows, cols)[r0:r0 + rows]
        else:
            self.b = raw.reshape(nrows, self.nb, 34 if ty == Q8 else 18)[r0:r0 + rows]

    # ---- block scale as f16 bits
    def get_d(self, r, kb):
        return self.b[r, kb, 0].astype(np.uint16) | (self.b[r, kb, 1].astype(np.uint16) << 8)

    def set_d(self, r, kb, bits):
        bits = np.asarray(bits, np.uint16)
        self.b[r, kb, 0] = (bits & 0xFF).astype(np.uint8)
        self.b[r, kb, 1] = (bits >> 8).astype(np.uint8)

    def zero(self, r, kb=slice(None)):
        """rows r x K blocks kb dequantise to exactly 0"""
        if self.ty == F16T:
            self.h.reshape(self.rows, self.nb, 32)[r, kb] = 0
        else:
            self.set_d(r, kb, np.zeros_like(self.get_d(r, kb)))

    def shift(self, r, n):
        """rows r times 2^n, exact while the scale (F16: the value) stays a normal f16; a block scale that would overflow is left alone"""
        if self.ty == F16T:
            v = self.h[r].view(np.float16).astype(F32) * F32(2.0 ** n)
            assert np.all(np.abs(v) < 65504)
            self.h[r] = v.astype(np.float16).view(np.uint16)
        else:
            old = self.get_d(r, slice(None))
            d = old.view(np.float16).astype(F32) * F32(2.0 ** n)
            fits = np.abs(d) < 65504                                       # a 2^15 scale of w-scales stays as it is
            self.set_d(r, slice(None), np.where(fits, np.where(fits, d, 0).astype(np.float16).view(np.uint16), old))

    def scale(self, r, factor):
        """rows r times any factor (negative: sign flip), through the block scales (F16: the values), rounded to f16"""
        if self.ty == F16T:
            self.h[r] = (self.h[r].view(np.float16).astype(np.float64) * factor).astype(np.float16).view(np.uint16)
        else:
            d = self.get_d(r, slice(None)).view(np.float16).astype(np.float64) * factor
            self.set_d(r, slice(None), d.astype(np.float16).view(np.uint16))

    def shrink(self, r, factor):
        """rows r times `factor` << 1 as far as the format goes: the scale first (down to one f16 ulp), then the quants"""
        if self.ty == F16T:
            self.h[r] = (self.h[r].view(np.float16).astype(np.float64) * factor).astype(np.float16).view(np.uint16)
            return
        d = self.get_d(r, slice(None)).view(np.float16).astype(np.float64) * factor
        ulp = 2.0 ** -24
        small = np.abs(d) < ulp
        rest = np.where(small, np.abs(d) / ulp, 1.0)                       # what the quants still have to take
        dn = np.where(small, np.copysign(ulp, d), d).astype(np.float16).view(np.uint16)
        self.set_d(r, slice(None), dn)
        if self.ty == Q8:
            q = self.b[r, :, 2:].view(np.int8).astype(np.float64) * rest[..., None]
            self.b[r, :, 2:] = np.rint(q).astype(np.int8).view(np.uint8)
        else:
            lo = ((self.b[r, :, 2:] & 0xF).astype(np.float64) - 8) * rest[..., None]
            hi = ((self.b[r, :, 2:] >> 4).astype(np.float64) - 8) * rest[..., None]
            self.b[r, :, 2:] = (np.rint(lo) + 8).astype(np.uint8) | ((np.rint(hi) + 8).astype(np.uint8) << 4)


def f32_tensor(m, name):
    return m.tensors[name][0].view(F32)


def part(m, l, which):
    """(tensor name, first row, rows) of q / k / v / o / gate / up / down of layer l (Phi-3: inside the fused tensors)."""
    c, p = m.cfg, "blk.%d." % l
    if c.arch == 4:
        if which in ("q", "k", "v"):
            r0 = {"q": 0, "k": c.q_dim, "v": c.q_dim + c.kv_dim}[which]
            return p + "attn_qkv.weight", r0, c.q_dim if which == "q" else c.kv_dim
        if which in ("gate", "up"):
            return p + "ffn_up.weight", 0 if which == "gate" else c.hidden, c.hidden
    if c.arch == 5 and which in ("gate", "up", "down"):
        return p + "ffn_%s_shexp.weight" % which, 0, None
    name = {"q": "attn_q", "k": "attn_k", "v": "attn_v", "o": "attn_output", "gate": "ffn_gate", "up": "ffn_up", "down": "ffn_down"}[which]
    return p + name + ".weight", 0, None


def matrices(m):
    """(Mat, quiet K block) of every matrix class: q k v o gate up down per layer, expert stacks, vocabulary, embedding."""
    c = m.cfg
    nb = c.dim // 32
    out = []
    for l in range(c.n_layers):
        for which, quiet in (("q", 3), ("k", 3), ("v", 3), ("o", 0), ("gate", nb - 1), ("up", nb - 1), ("down", 5)):
            a = Mat(m, *part(m, l, which))
            a.big = 0x7800 if which in ("q", "k", "o", "down") else 0x5C00
            if which == "up":
                a.big_row += 32             # not the row of gate's large scale: their product feeds a quantised activation
            out.append((a, quiet))
        if c.arch == 5:
            p, mh = "blk.%d." % l, c.moe_hidden
            for e in (0, MOE_EXPERT, c.n_experts - 1):
                for a, quiet in ((Mat(m, p + "ffn_gate_exps.weight", e * mh, mh), nb - 1), (Mat(m, p + "ffn_up_exps.weight", e * mh, mh), nb - 1),
                                 (Mat(m, p + "ffn_down_exps.weight", e * c.dim, c.dim), 3)):
                    a.big = 0x5C00
                    out.append((a, quiet))
                out[-2][0].big_row -= 32
    if not c.tied:
        out.append((Mat(m, "output.weight"), 1))
    emb = Mat(m, "token_embd.weight")
    emb.big = 0x5C00                        # 2^8: as an embedding row it is the residual stream itself
    out.append((emb, 1))
    return out


# ------------------------------------------------------------------ the edits
def act_blocks(m):
    c = m.cfg
    nb = c.dim // 32
    plans = {"attn_norm": {1: 0.0, 2: ROUND0, 3: SUBN, nb - 1: OUTLIER},
             "ffn_norm": {0: OUTLIER, 1: ROUND0, nb - 2: 0.0, nb - 1: SUBN},
             "output_norm": {0: ROUND0, 1: SUBN, 2: OUTLIER, nb - 1: 0.0}}
    for name in m.tensors:
        for key, plan in plans.items():
            if name.endswith(key + ".weight"):
                g = f32_tensor(m, name).reshape(nb, 32)
                for b, f in plan.items():
                    g[b] *= F32(f)
        if name.endswith("attn_q_norm.weight") or name.endswith("attn_k_norm.weight"):
            g = f32_tensor(m, name)
            g[5] = 0
            g[9] *= F32(QN_LARGE if "q_norm" in name else KN_LARGE)
    Mat(m, "token_embd.weight").zero(ZERO_TOKEN)


def inner_act_blocks(m):
    c = m.cfg
    for l in range(c.n_layers):
        v = Mat(m, *part(m, l, "v"))
        v.zero(slice(0, 32))
        if c.arch in (2, 5):                       # MoE: the whole bias, so that ZERO_TOKEN at position 0 keeps x = 0 and v = 0 in every layer (sink_head)
            f32_tensor(m, "blk.%d.attn_v.bias" % l)[:32 if c.arch == 2 else None] = 0
        if c.kv_dim // 32 >= 4:
            v.shrink(slice(32, 64), 2.0 ** -10)
            v.shrink(slice(64, 96), 2.0 ** -19)
        pairs = [(Mat(m, *part(m, l, "gate")), Mat(m, *part(m, l, "up")), c.hidden)]
        if c.arch == 5:
            p, mh = "blk.%d." % l, c.moe_hidden
            pairs.append((Mat(m, p + "ffn_gate_exps.weight", MOE_EXPERT * mh, mh), Mat(m, p + "ffn_up_exps.weight", MOE_EXPERT * mh, mh), mh))
        for g, u, n in pairs:
            u.zero(slice(32, 64))
            for i, (ue, ge_) in enumerate(UP_LADDER if n // 32 >= 8 else UP_LADDER_NARROW):
                rows = slice(64 + 32 * i, 96 + 32 * i)
                u.shrink(rows, 2.0 ** ue)
                if ge_:
                    g.shrink(rows, 2.0 ** ge_)


def w_scales(m):
    for a, quiet in matrices(m):
        last, lb = a.rows - 1, a.nb - 1
        a.set_d(0, 0, 0x0000)
        a.set_d(0, lb, 0x0001)
        a.set_d(1, 0, 0x03FF)
        a.set_d(1, lb, 0x0400)
        a.set_d(last, lb, 0x0000)
        if a.ty == Q8:
            a.set_d(last, 0, a.get_d(last, 0) ^ 0x8000)
            a.set_d(7, slice(None), a.get_d(7, slice(None)) ^ 0x8000)
        a.set_d(a.big_row, min(quiet, lb), a.big)                # 2^15; + 9: not a row that is itself an edited K position downstream


def flat_pattern():
    return np.where(np.arange(32) % 2 == 0, 127, -127).astype(np.int8)


def w_quants(m):
    c = m.cfg
    nb = c.dim // 32
    for a, _ in matrices(m):
        lb = a.nb - 1
        if a.ty == Q8:
            a.b[2, 0, 2:] = np.full(32, -128, np.int8).view(np.uint8)
            a.b[2, lb, 2:] = np.full(32, 127, np.int8).view(np.uint8)
            a.b[3, a.nb // 2, 2:] = flat_pattern().view(np.uint8)
        else:
            a.b[2, 0, 2:] = 0x00
            a.b[2, lb, 2:] = 0xFF
    if m.wtype != Q8:
        return
    # the flat token: |q| = 127 throughout block nb-1, attn_norm of layer 0 flat on that block, attn_q rows matched to its signs
    emb = Mat(m, "token_embd.weight")
    emb.b[FLAT_TOKEN, nb - 1, 2:] = flat_pattern().view(np.uint8)
    g = f32_tensor(m, "blk.0.attn_norm.weight").reshape(nb, 32)
    g[nb - 1] = g[nb - 1, 0]
    q = Mat(m, *part(m, 0, "q"))
    q.b[4, nb - 1, 2:] = flat_pattern().view(np.uint8)                       # isum = +32 * 127 * 127
    q.b[5, nb - 1, 2:] = np.full(32, -128, np.int8).view(np.uint8)           # isum = 0: +-127 * -128 cancel pairwise
    q.b[6, nb - 1, 2:] = np.where(np.arange(32) % 2 == 0, -128, 127).astype(np.int8).view(np.uint8)    # isum = -16 * 127 * 255


def f16_values(m):
    sub = np.arange(1, 17, dtype=np.uint16) * 61                             # 16 subnormals, 0x003D .. 0x03D0
    zeros = np.array([0x8000, 0x0000] * 4, np.uint16)
    for a, _ in matrices(m):
        h, last, K = a.h, a.rows - 1, a.cols
        h[0, 0:16] = sub
        h[0, 16:24] = zeros
        h[0, K - 8:K] = 0x7BFF
        h[last, 0:8] = 0x0400
        h[last, K - 16:K] = sub | 0x8000
        h[last, K - 24:K - 16] = zeros
        h[1, 7], h[1, 40], h[1, K - 1] = 0x8000, 0x0001, 0x83FF
        h[2, 3], h[2, 100] = 0x0400, 0xFBFF


def peaked_attn(m):
    """Alone: exact power-of-two shifts of the attn_q block scales (F16: values), PEAK_SHIFT_ALONE.  With act-blocks the OUTLIER block drives q and k to ~10^3 and every score gap to ~10^5: the K rows under heads 4 .. 6 and the Q rows
    of heads 5 and 6 then lose that K block (d = 0, exact), which leaves head 4 far out, brings head 5 to gaps of ~10^2 and, shrunk by another 2^-8, head 6 to ~10^-1."""
    c = m.cfg
    nb, hs, kvmul = c.dim // 32, c.head_size, c.n_heads // c.n_kv_heads
    with_act = "act-blocks" in m.edits
    for l in range(c.n_layers):
        q, k = Mat(m, *part(m, l, "q")), Mat(m, *part(m, l, "k"))
        if with_act:
            for kvh in sorted({h // kvmul for h in (4, 5, 6, SINK_HEAD) if h < c.n_heads}):
                k.zero(slice(kvh * hs, (kvh + 1) * hs), nb - 1)
            q.zero(slice(5 * hs, 8 * hs), nb - 1)
            q.shrink(slice(6 * hs, 7 * hs), 2.0 ** -8)
        for head, n in (PEAK_SHIFT if with_act else PEAK_SHIFT_ALONE).items():
            if head < c.n_heads:
                q.shift(slice(head * hs, (head + 1) * hs), n)


def moe_router(m):
    c = m.cfg
    for l in range(c.n_layers):
        r = f32_tensor(m, "blk.%d.ffn_gate_inp.weight" % l).reshape(c.n_experts, c.dim)
        r[1] *= F32(4.0)
        r[2] = r[1]
        r[MOE_EXPERT] *= F32(1000.0)


_APPLY = {"act-blocks": act_blocks, "inner-act-blocks": inner_act_blocks, "w-scales": w_scales, "w-quants": w_quants,
          "f16-values": f16_values, "peaked-attn": peaked_attn, "moe-router": moe_router}


def sink_head(m):
    """An f16-subnormal block INTO wo on shapes with two 32-row groups of V (one zero, one ordinary; no third to shrink).  ZERO_TOKEN at
    position 0 keeps x = 0 through every layer (no bias left on its way), so its V row is 0 everywhere.  At position 1 head SINK_HEAD
    sees two scores; its output is sigmoid(s1 - s0) * v1.  Layer by layer the head's attn_q rows (and bias) are scaled by the factor
    that makes amax of that output SINK_TARGET, taken from a two-token run of the NumPy oracle on the model built so far; the scale is
    applied to f16 block scales, which moves s1 - s0 by ~1e-3 of itself, far inside the window of +-3.4."""
    from oracle import oracle_np
    c = m.cfg
    hs, kvh = c.head_size, SINK_HEAD // (c.n_heads // c.n_kv_heads)
    for l in range(c.n_layers):
        o = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope)
        o.attn_taps = []
        for pos, t in enumerate((ZERO_TOKEN, FLAT_TOKEN)):
            o.forward(t, pos, want_logits=False)
        score = [sc for ll, h, pos, sc in o.attn_taps if (ll, h, pos) == (l, SINK_HEAD, 1)][0]
        vmax = float(np.max(np.abs(o.vc[l, 1, kvh * hs:(kvh + 1) * hs])))
        gap = float(score[1]) - float(score[0])
        assert float(np.max(np.abs(o.vc[l, 0]))) == 0 and vmax > 0 and gap != 0, (l, vmax, gap)
        f = -np.log(vmax / SINK_TARGET) / gap
        rows = slice(SINK_HEAD * hs, (SINK_HEAD + 1) * hs)
        Mat(m, *part(m, l, "q")).scale(rows, f)
        if c.arch in (2, 5):
            b = f32_tensor(m, "blk.%d.attn_q.bias" % l)
            b[rows] = (b[rows].astype(np.float64) * f).astype(F32)


def make_edge_model(cfg_name, wtype=8, seed=7, edits="all", **cfg_overrides):
    pkg = ge.load_package()
    base = pkg.synth.CONFIGS[cfg_name]
    cfg = pkg.synth.ModelConfig(**{**base.__dict__, **cfg_overrides}) if cfg_overrides else base
    m = pkg.synth.make_numpy(cfg, wtype=wtype, seed=seed)
    m.edits = edits_for(wtype, cfg.arch, edits)
    # fixed order, whatever order the caller names them in; inner-act-blocks after the weight edits: its zero rows must stay zero
    for name in ("act-blocks", "w-scales", "w-quants", "inner-act-blocks", "f16-values", "peaked-attn", "moe-router"):
        if name in m.edits:
            _APPLY[name](m)
    if wtype == Q8 and cfg.arch in (0, 3, 5) and {"act-blocks", "inner-act-blocks", "peaked-attn"} <= set(m.edits):
        sink_head(m)
    return m


def edge_tokens(pkg, m, n):
    """The token list of the edge tests: the bench stream with ZERO_TOKEN at positions 0 (the sink of sink_head), 5 and 9 (as a query it ties
    every score at +-0) and FLAT_TOKEN at 1 and 7."""
    t = list(pkg.javarand.bench_tokens(m.cfg.vocab, n))
    for p, tok in ((0, ZERO_TOKEN), (1, FLAT_TOKEN), (5, ZERO_TOKEN), (7, FLAT_TOKEN), (9, ZERO_TOKEN)):
        if p < n:
            t[p] = tok
    return t


def routed_tokens(m, n, first=MOE_EXPERT):
    """n token ids which, alone at position 0, make the same expert choices as each other in every layer, and the choice of the last layer
    (a list of expert ids).  With `first` every layer's choice must start with it; with first = None it is the first set of choices that
    n tokens share.  (By the NumPy oracle.)"""
    from oracle import oracle_np
    o = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope)
    groups = {}
    for t in range(m.cfg.vocab):
        o.moe_taps = []
        o.forward(t, 0, want_logits=False)
        key = tuple(tuple(sel) for _, sel, _ in o.moe_taps)
        if first is None or all(sel[0] == first for sel in key):
            g = groups.setdefault(key, [])
            g.append(t)
            if len(g) == n:
                return g, list(key[-1])
    raise AssertionError("no %d tokens share their expert choices (first = %s): %s" % (n, first, sorted(len(v) for v in groups.values())))
