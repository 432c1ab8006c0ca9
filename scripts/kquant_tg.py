"""tg128 of a Llama-3-8B-shaped random model in the Q4_K_M mix (Q4_K matrices; Q6_K for attn_v, every second ffn_down and output)
or, with --mix q5_k_m, the Q5_K_M mix (Q5_K in Q4_K's place),
once converted to Q8_0 at load (the default plan) and once with the K-quant tensors native in HBM (GL3_FLAG_KQUANT_NATIVE).

bench.py's tg protocol (decode steps from an empty cache, logits to the host every step): 1 warm-up and --reps timed repetitions
per plan, the two plans alternated inside one invocation, their logits compared for equality.  Also the per-class device times of
instrumented steps and the algorithmic bytes per token of both plans, computed from the shapes.  Prints one JSON line.

    python scripts/kquant_tg.py [--layers 32] [--reps 5] [--mix q4_k_m|q5_k_m]
    rocprofv3 --kernel-trace --stats -- python scripts/kquant_tg.py --reps 1        # per-kernel times
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Q8_0, Q4_K, Q5_K, Q6_K = 8, 12, 13, 14
BLOCK_BYTES = {Q4_K: 144, Q5_K: 176, Q6_K: 210}            # per 256 elements
MIXES = {"q4_k_m": Q4_K, "q5_k_m": Q5_K}        # the type of every matrix that is not Q6_K


def ggml_type(name, mix="q4_k_m"):
    layer = int(name.split(".")[1]) if name.startswith("blk.") else 0
    return Q6_K if ("attn_v" in name or name == "output.weight" or ("ffn_down" in name and layer % 2 == 0)) else MIXES[mix]


class KqModel:
    """Streams the tensors of the model in file order, generated from a seed; convert = as the default loader would upload them."""

    def __init__(self, cfg, synth, lib, seed, convert, mix="q4_k_m", types=None):
        self.cfg, self.wtype, self.rope = cfg, Q8_0, synth.model_rope(cfg)
        self._synth, self._lib, self._seed, self._convert = synth, lib, seed, convert
        self.types = types or (lambda name, cols: ggml_type(name, mix))      # types(name, cols) -> ggml type; Q8_0 where a row holds no super-block

    def tensor_items(self):
        rng = np.random.default_rng(self._seed)
        for name, rows, cols, ty, kind in self._synth.tensor_specs(self.cfg, Q8_0):
            if kind != "mat":
                yield name, ((rng.standard_normal(rows * cols, dtype=np.float32) * np.float32(0.02) + np.float32(1)).view(np.uint8), ty, rows, cols)
                continue
            t, nb = self.types(name, cols), rows * cols // 256
            if t == Q8_0:                               # random int8 codes under small f16 scales, the same in both plans
                b = rng.integers(0, 256, (rows * cols // 32, 34), dtype=np.uint8)
                b[:, 0:2] = (np.abs(rng.standard_normal(len(b))) * 2e-4 + 2e-5).astype(np.float16).view(np.uint8).reshape(len(b), 2)
                yield name, (b.reshape(-1), Q8_0, rows, cols)
                continue
            b = rng.integers(0, 256, (nb, BLOCK_BYTES[t]), dtype=np.uint8)
            step = 0.5 if t == Q5_K else 1.0           # 32 levels over the range Q4_K covers with 16: the fifth bit buys resolution
            d = ((np.abs(rng.standard_normal(nb)) * 2e-3 + 2e-4) * step).astype(np.float16).view(np.uint8).reshape(nb, 2)
            if t == Q6_K:
                b[:, 208:210] = d
            else:
                b[:, 0:2] = d
                b[:, 2:4] = (np.abs(rng.standard_normal(nb)) * 8e-3).astype(np.float16).view(np.uint8).reshape(nb, 2)
            raw = b.reshape(-1)
            if self._convert:
                q8 = np.empty(rows * cols // 32 * 34, np.uint8)
                assert self._lib.gl3_kquant_to_q8_0(t, raw.ctypes.data_as(C.c_void_p), rows * cols, q8.ctypes.data_as(C.c_void_p)) == 0
                raw, t = q8, Q8_0
            yield name, (raw, t, rows, cols)


def tg_compare(plans, toks, n_gen, reps):
    """tg of the "converted" and the "native" plan alternated: 1 warm-up and `reps` timed repetitions each, the last logits of every repetition
    compared; then 8 instrumented steps per plan.  -> ({plan: figures}, outputs equal, outputs finite)"""
    def rep(plan):
        t1 = time.perf_counter()
        for i in range(n_gen):
            logits = plan.forward_decode(toks[i], i, copy=False)
        return time.perf_counter() - t1, logits.copy()

    samples, equal, finite = {k: [] for k in plans}, True, True
    for r in range(reps + 1):                          # repetition 0 is the warm-up
        last = {}
        for k, plan in plans.items():
            s, last[k] = rep(plan)
            if r:
                samples[k].append(n_gen / s)
        equal = equal and bool(np.array_equal(last["converted"], last["native"]))
        finite = finite and bool(np.isfinite(last["converted"]).all())
    out = {}
    for k, plan in plans.items():
        acc, n_prof = None, 8
        for i in range(n_prof):
            kt = plan.profile_decode(toks[64 + i], 64 + i)
            if acc is None:
                acc = kt
            else:
                for name in kt:
                    for f in ("ms", "launches", "bytes"):
                        acc[name][f] += kt[name][f]
        s = samples[k] or [0.0]
        out[k] = dict(tok_s=round(float(np.mean(s)), 2), samples_tok_s=[round(x, 2) for x in s], spread_tok_s=round(max(s) - min(s), 2),
                      weight_bytes_in_hbm=plan.weight_bytes(),
                      kernel_classes={n: dict(us_per_token=round(v["ms"] / n_prof * 1e3, 1), launches_per_token=v["launches"] // n_prof,
                                              gbs=round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1) if v["ms"] > 0 else None)
                                      for n, v in acc.items() if v["launches"]})
    return out, equal, finite


def moe_mix(name, cols):
    """the K-quant mix of the Qwen2-MoE scripts: Q4_K everywhere, Q6_K for attn_v, ffn_down* and output, Q8_0 where K is no multiple of 256"""
    return Q8_0 if cols % 256 else Q6_K if ("attn_v" in name or "ffn_down" in name or name == "output.weight") else Q4_K


def moe_plans(cfg, synth, hip, plan_mod, **kw):
    """the converted and the native plan (GL3_FLAG_KQUANT_NATIVE_MOE) of a Qwen2-MoE shape in that mix"""
    return {"converted": plan_mod.HipMasterPlan(KqModel(cfg, synth, hip.lib(), 42, True, types=moe_mix), **kw),
            "native": plan_mod.HipMasterPlan(KqModel(cfg, synth, hip.lib(), 42, False, types=moe_mix), flags=hip.FLAG_KQUANT_NATIVE_MOE, **kw)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-gen", type=int, default=128)
    ap.add_argument("--mix", choices=sorted(MIXES), default="q4_k_m")
    args = ap.parse_args()
    import __graft_entry__ as ge
    from importlib import import_module
    pkg = ge.load_package()
    synth = pkg.synth
    plan_mod, hip = import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")
    cfg = synth.CONFIGS["llama-3-8b"]
    cfg = synth.ModelConfig(**{**cfg.__dict__, "ctx": args.n_gen + 8, "n_layers": args.layers})
    t0 = time.time()
    plans = {"converted": plan_mod.HipMasterPlan(KqModel(cfg, synth, hip.lib(), 42, True, args.mix)),
             "native": plan_mod.HipMasterPlan(KqModel(cfg, synth, hip.lib(), 42, False, args.mix), flags=hip.FLAG_KQUANT_NATIVE)}
    setup_s = time.time() - t0
    toks = pkg.javarand.bench_tokens(cfg.vocab, args.n_gen)
    measured, equal, finite = tg_compare(plans, toks, args.n_gen, args.reps)
    d, L = cfg.dim, cfg.n_layers
    mats = [(n, r, c) for n, r, c, ty, kind in synth.tensor_specs(cfg, Q8_0) if kind == "mat" and n != "token_embd.weight"]
    bpe = {t: b / 256 for t, b in BLOCK_BYTES.items()}
    other = d * 34 / 32 + (2 * L + 1) * d * 4 + 2 * L * cfg.kv_dim * 4 * ((args.n_gen - 1) / 2.0 + 2) + cfg.vocab * 4
    out = dict(metric="tg%d tokens/s" % args.n_gen, unit="tokens/s", n_gpus=1, data="synthetic", outputs_equal=equal, outputs_finite=finite, setup_s=round(setup_s, 1),
               config=dict(workload="Llama-3-8B shape, %s mix, %d layers, random weights" % (args.mix.upper(), L), reps=args.reps))
    for k in plans:
        weights = sum(r * c * (34 / 32 if k == "converted" else bpe[ggml_type(n, args.mix)]) for n, r, c in mats)
        out[k] = dict(measured[k], algorithmic_bytes_per_token=int(weights + other))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
