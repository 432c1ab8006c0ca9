"""HipMasterPlan — host-side mirror of the reference's plan interface over the C-ABI.

Mirrors ``interface TornadoVMMasterPlan`` (J/tornadovm/TornadoVMMasterPlan.java:30-85) and its
BatchPrefillDecode subclass (J/tornadovm/TornadoVMMasterPlanBatchPrefillDecode.java:107-168) with
the reference's method names, so callers read like the Java engines:

    plan = HipMasterPlan.initializeTornadoVMPlan(model, prefill_batch_size=512)   # ctor + copy-in
    plan.tornadoVMForwardBatchPrefill(tokens, start_pos)                          # no logits
    logits = plan.tornadoVMForwardDecode(token, position)                         # f32[vocab]
    plan.freeTornadoExecutionPlan()

Differences that the C-ABI makes explicit: the token id is an argument (the
reference passes the embedding row through State.embeddingX) and logits are returned, not left in
State.wrapLogits.  Unsupported model x quant x mode combinations raise Gl3Error(GL3_E_UNSUPPORTED)
where the reference throws UnsupportedOperationException (ForwardPlanFactory.java:84-86).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import hip


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


# gl3_token_score (include/gpullama3_hip.h): 16 bytes per row
SCORE_DTYPE = np.dtype([("prob", np.float32), ("logit", np.float32), ("max", np.float32), ("sum", np.float32)])
# gl3_verify_result: 8 bytes per run
VERIFY_DTYPE = np.dtype([("accepted", np.int32), ("token", np.int32)])


class HipMasterPlan:
    def __init__(self, model, prefill_batch_size: int = 1, device: int = 0, tp_rank: int = 0, tp_size: int = 1,
                 flags: int = 0, unique_id: bytes | None = None, local_group=None, n_seqs: int = 1, p2p_exchange=None):
        """model: synth.SynthModel-like — cfg, tensors {gguf name: (raw uint8, ggml_type, rows, cols)}, rope (cr, ci).

        Tensor parallel (tp_size > 1), one of: ``p2p_exchange`` — a callable that takes this rank's 64-byte IPC handle and
        returns the handles of ALL ranks in rank order (e.g. torch.distributed.all_gather_object): peer-write all-gathers over
        xGMI, the default transport; ``unique_id`` — RCCL fall-back; ``local_group`` — ranks are threads of this process (tests)."""
        L = hip.lib()
        c = model.cfg
        self.cfg = c
        self._ctx = C.c_void_p()
        d = hip.ModelDesc(C.sizeof(hip.ModelDesc), c.arch, c.dim, c.hidden, c.n_layers, c.n_heads, c.n_kv_heads,
                          c.head_size, c.vocab, c.ctx, c.rms_eps, model.wtype, prefill_batch_size, device, tp_rank,
                          tp_size, flags, n_seqs, getattr(c, "embedding_scale", 1.0), getattr(c, "attention_scale", 0.0),
                          getattr(c, "residual_scale", 1.0), getattr(c, "logit_scale", 1.0),
                          getattr(c, "n_experts", 0), getattr(c, "n_experts_used", 0), getattr(c, "moe_hidden", 0))
        hip.check(L.gl3_create(C.byref(d), C.byref(self._ctx)))
        self.tp_size, self.tp_rank = tp_size, tp_rank
        self.max_batch = prefill_batch_size
        try:
            if local_group is not None:
                hip.check(L.gl3_tp_attach_local(self._ctx, local_group), self._ctx)
            elif p2p_exchange is not None:
                mine = C.create_string_buffer(64)
                hip.check(L.gl3_tp_p2p_handle(self._ctx, mine, 64), self._ctx)
                every = list(p2p_exchange(mine.raw))
                assert len(every) == tp_size and all(len(h) == 64 for h in every), "p2p_exchange must return tp_size 64-byte handles"
                blob = C.create_string_buffer(b"".join(every), 64 * tp_size)
                hip.check(L.gl3_tp_p2p_attach(self._ctx, blob, 64 * tp_size), self._ctx)
            elif tp_size > 1 or flags & hip.FLAG_FORCE_RCCL:
                assert unique_id is not None, "tensor parallel plan needs the RCCL unique id from rank 0"
                buf = C.create_string_buffer(unique_id, len(unique_id))
                hip.check(L.gl3_tp_init(self._ctx, buf, len(unique_id)), self._ctx)
            for name, t in model.tensor_items():
                raw, ty = t[0], t[1]
                if name.startswith("blk."):
                    _, l, rest = name.split(".", 2)
                    tid, layer = hip.T_IDS[rest], int(l)
                    if c.arch == 4 and rest == "ffn_up.weight":        # phi3: the fused gate | up tensor
                        tid = hip.T_W13
                else:
                    tid, layer = hip.T_IDS[name], 0
                raw = np.ascontiguousarray(raw)
                hip.check(L.gl3_upload_tensor(self._ctx, tid, layer, _p(raw), raw.nbytes, ty), self._ctx)
            cr, ci = model.rope
            hip.check(L.gl3_upload_rope(self._ctx, _p(cr), _p(ci), cr.size), self._ctx)
            self.forceCopyInReadOnlyData()
        except Exception:
            self.freeTornadoExecutionPlan()
            raise
        self._arg = C.c_int32()
        self._pin_logits()

    def _pin_logits(self):
        """The logits buffer is reused on every step: page-lock it once so the D2H copy lands in it directly.  Registration pins
        whole pages, so the buffer is an anonymous mapping of its own (page-aligned, padded to whole pages) — never a slice
        of the C heap, whose pages it would share with unrelated allocations."""
        import mmap
        nbytes = (self.cfg.vocab * 4 + 4095) & ~4095
        self._logits_map = mmap.mmap(-1, nbytes)
        self._logits = np.frombuffer(self._logits_map, np.float32, self.cfg.vocab)
        try:
            hip.check(hip.lib().gl3_pin_host_buffer(self._ctx, _p(self._logits), nbytes), self._ctx)
        except hip.Gl3Error:
            pass                                      # not fatal: the plan falls back to its own staging buffer

    @classmethod
    def from_gguf(cls, path: str, prefill_batch_size: int = 1, ctx: int = 0, device: int = 0, flags: int = 0, n_seqs: int = 1):
        """Native loader (gl3_load_gguf): the library mmaps the GGUF file, reads the config keys the reference loaders read
        (LlamaModelLoader.java:47-69, Qwen3ModelLoader.java:48-79), uploads every tensor and builds the RoPE table itself."""
        from . import synth
        L = hip.lib()
        self = cls.__new__(cls)
        g = C.c_void_p()
        hip.check_gguf(L.gl3_gguf_open(path.encode(), C.byref(g)))
        try:
            d = hip.ModelDesc()
            d.ctx = ctx
            theta = C.c_float()
            hip.check_gguf(L.gl3_gguf_model_desc(g, C.byref(d), C.byref(theta)), g)
            name = C.c_char_p()
            nm = name.value.decode() if L.gl3_gguf_meta_string(g, b"general.name", C.byref(name)) == 0 else os.path.basename(path)
            tied = True
            for i in range(L.gl3_gguf_tensor_count(g)):
                tn = C.c_char_p()
                L.gl3_gguf_tensor_info(g, i, C.byref(tn), None, None, None, None)
                if tn.value == b"output.weight":
                    tied = False
            # Devstral 2 ("mistral3"): the native loader uploads the YaRN table, so the host-side config must describe it too — an
            # oracle or KV comparison built from plan.cfg would otherwise compute the plain table (r4 advisor finding)
            ga = C.c_char_p()
            gguf_arch = ga.value.decode() if L.gl3_gguf_meta_string(g, b"general.architecture", C.byref(ga)) == 0 else None
            yf, ybf, ybs, ylm, yoc = C.c_float(), C.c_float(), C.c_float(), C.c_float(), C.c_int32()
            yr = L.gl3_gguf_yarn_params(g, C.byref(yf), C.byref(ybf), C.byref(ybs), C.byref(ylm), C.byref(yoc))
            if yr < 0:
                raise hip.Gl3Error(hip.E_ARG, "mistral3.rope.scaling: factor and original_context_length must be finite and > 0")
            yarn = (yf.value, ybf.value, ybs.value, ylm.value, yoc.value) if yr > 0 else None
        finally:
            L.gl3_gguf_close(g)
        self.cfg = synth.ModelConfig(nm, d.arch, d.dim, d.hidden, d.n_layers, d.n_heads, d.n_kv_heads, d.head_size, d.vocab, d.ctx,
                                     d.rms_eps, float(theta.value), tied, n_experts=d.n_experts, n_experts_used=d.n_experts_used,
                                     moe_hidden=d.moe_hidden, yarn=yarn, gguf_arch=gguf_arch if gguf_arch == "mistral3" else None)
        opts = hip.ModelDesc()
        opts.struct_size = C.sizeof(hip.ModelDesc)
        opts.ctx, opts.max_batch, opts.device, opts.tp_size, opts.flags, opts.n_seqs = ctx, prefill_batch_size, device, 1, flags, n_seqs
        self._ctx = C.c_void_p()
        hip.check_gguf(L.gl3_load_gguf(path.encode(), C.byref(opts), C.byref(self._ctx)))
        self.tp_size, self.tp_rank, self.max_batch = 1, 0, prefill_batch_size
        self._arg = C.c_int32()
        self._pin_logits()
        return self

    # ---- reference-named interface -------------------------------------------------------------
    @classmethod
    def initializeTornadoVMPlan(cls, model, prefill_batch_size: int = 1, **kw) -> "HipMasterPlan":
        """TornadoVMMasterPlan.initializeTornadoVMPlan(state, model) :55-70 — the plan flavour is picked from
        llama.prefillBatchSize: > 1 allocates the batched-prefill (MFMA) buffers."""
        return cls(model, prefill_batch_size=prefill_batch_size, **kw)

    def forceCopyInReadOnlyData(self):
        hip.check(hip.lib().gl3_finalize(self._ctx), self._ctx)

    def tornadoVMForwardDecode(self, token: int, position: int) -> np.ndarray:
        """One decode step; returns the logits (host-visible on return, like state.wrapLogits)."""
        return self.forward_decode(token, position)

    def tornadoVMForwardPrefill(self, token: int, position: int):
        """TornadoVMMasterPlanPrefillDecode.tornadoVMForwardPrefill(position): one token, logits skipped."""
        t = np.array([token], np.int32)
        hip.check(hip.lib().gl3_forward_prefill(self._ctx, _p(t), 1, position), self._ctx)

    def tornadoVMForwardBatchPrefill(self, tokens, start_pos: int):
        """TornadoVMMasterPlanBatchPrefillDecode.tornadoVMForwardBatchPrefill(): one chunk, logits skipped."""
        t = np.ascontiguousarray(tokens, np.int32)
        hip.check(hip.lib().gl3_forward_prefill(self._ctx, _p(t), t.size, start_pos), self._ctx)

    def prefill_seq(self, seq: int, tokens, start_pos: int = 0):
        """Prefill sequence `seq` (its own KV cache) in chunks of max_batch."""
        tokens = list(tokens)
        b = max(1, self.max_batch)
        for off in range(0, len(tokens), b):
            t = np.ascontiguousarray(tokens[off:off + b], np.int32)
            hip.check(hip.lib().gl3_forward_prefill_seq(self._ctx, seq, _p(t), t.size, start_pos + off), self._ctx)

    def forward_decode_batch(self, tokens, seq_ids, positions, want_logits: bool = True):
        """Static batched decode: one step for n independent sequences -> (logits [n][vocab] or None, greedy ids [n])."""
        t = np.ascontiguousarray(tokens, np.int32); s = np.ascontiguousarray(seq_ids, np.int32); p = np.ascontiguousarray(positions, np.int32)
        n = t.size
        logits = np.empty((n, self.cfg.vocab), np.float32) if want_logits else None
        ids = np.empty(n, np.int32)
        hip.check(hip.lib().gl3_forward_decode_batch(self._ctx, _p(t), _p(s), _p(p), n, _p(logits) if want_logits else None, _p(ids)), self._ctx)
        return logits, ids

    @staticmethod
    def _per_row(v, n):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (n,)))

    def forward_decode_batch_sample(self, tokens, seq_ids, positions, temperature, topp, coins) -> np.ndarray:
        """Static batched decode + the reference's sampler for every row on the device -> sampled ids [n].  temperature / topp /
        coins: one entry per row (scalars broadcast); coins[i] = rng.nextFloat(1f) from row i's own generator (ignored for
        temperature 0)."""
        t = np.ascontiguousarray(tokens, np.int32); s = np.ascontiguousarray(seq_ids, np.int32); p = np.ascontiguousarray(positions, np.int32)
        n = t.size
        te, tp, co = self._per_row(temperature, n), self._per_row(topp, n), self._per_row(coins, n)
        ids = np.empty(n, np.int32)
        hip.check(hip.lib().gl3_forward_decode_batch_sample(self._ctx, _p(t), _p(s), _p(p), n, _p(te), _p(tp), _p(co), _p(ids)), self._ctx)
        return ids

    def forward_decode_batch_chain(self, tokens, seq_ids, positions, k: int, temperature=0.0, coins=None, k_rows=None,
                                   target: "HipMasterPlan" = None, slots=None) -> np.ndarray:
        """k static-batched decode steps behind one wait, every row's id fed to its next step on the device
        (gl3_forward_decode_batch_chain): what k forward_decode_batch_sample calls over the rows with k_rows[i] > j return, int32[k][n], -1
        where a row has no step.  temperature: per row (a scalar broadcasts), 0 = greedy; coins: f32[k][n] or None when every row is greedy;
        k_rows: int32[n] non-increasing from k, or None (every row k steps); target / slots: row i's step j goes into slot slots[i] + j of
        that plan's draft table (slots[i] = -1: none), as draft_probs_put_row."""
        t = np.ascontiguousarray(tokens, np.int32); s = np.ascontiguousarray(seq_ids, np.int32); p = np.ascontiguousarray(positions, np.int32)
        n = t.size
        assert s.size == n and p.size == n
        te = self._per_row(temperature, n)
        co = np.ascontiguousarray(coins, np.float32) if coins is not None else None
        assert co is None or co.shape == (k, n)      # the C entry reads k * n coins: it cannot see a shorter array
        kr = np.ascontiguousarray(k_rows, np.int32) if k_rows is not None else None
        sl = np.ascontiguousarray(slots, np.int32) if slots is not None else None
        assert (kr is None or kr.shape == (n,)) and (sl is None or sl.shape == (n,))
        out = np.zeros((max(k, 1), n), np.int32)
        hip.check(hip.lib().gl3_forward_decode_batch_chain(self._ctx, _p(t), _p(s), _p(p), n, k, _p(kr) if kr is not None else None, _p(te),
                                                           _p(co) if co is not None else None, target._ctx if target is not None else None,
                                                           _p(sl) if sl is not None else None, _p(out)), self._ctx)
        return out[:k]

    def _mixed_args(self, tokens, seq_ids, positions, want_logits):
        """The arrays of a mixed step and its number of output rows (want_logits None: the last row of every run)."""
        t = np.ascontiguousarray(tokens, np.int32); s = np.ascontiguousarray(seq_ids, np.int32); p = np.ascontiguousarray(positions, np.int32)
        assert t.size == s.size == p.size
        if want_logits is None:
            w, n_out = None, (int(np.count_nonzero(s[1:] != s[:-1])) + 1 if s.size else 0)
        else:
            w = np.ascontiguousarray(np.asarray(want_logits) != 0, np.int8)
            assert w.size == t.size
            n_out = int(np.count_nonzero(w))
        return t, s, p, w, n_out

    def forward_batch(self, tokens, seq_ids, positions, want_logits=None, logits: bool = True):
        """Mixed batched step (gl3_forward_batch): rows = runs of consecutive rows of one sequence at consecutive positions, a run of one
        row is a decode row, a longer one a prompt chunk -> (logits [n_out][vocab] or None, greedy ids [n_out]) of the rows flagged in
        want_logits (None: the last row of every run).  logits=False skips the logits copy."""
        t, s, p, w, n_out = self._mixed_args(tokens, seq_ids, positions, want_logits)
        lg = np.empty((n_out, self.cfg.vocab), np.float32) if logits and n_out else None
        ids = np.empty(n_out, np.int32)
        hip.check(hip.lib().gl3_forward_batch(self._ctx, _p(t), _p(s), _p(p), _p(w) if w is not None else None, t.size,
                                              _p(lg) if lg is not None else None, _p(ids) if n_out else None), self._ctx)
        return lg, ids

    def forward_batch_sample(self, tokens, seq_ids, positions, temperature, topp, coins, want_logits=None) -> np.ndarray:
        """Mixed batched step + the reference's sampler for every OUTPUT row on the device -> sampled ids [n_out].  temperature / topp /
        coins: one entry per output row (scalars broadcast), as in forward_decode_batch_sample."""
        t, s, p, w, n_out = self._mixed_args(tokens, seq_ids, positions, want_logits)
        te, tp, co = self._per_row(temperature, n_out), self._per_row(topp, n_out), self._per_row(coins, n_out)
        ids = np.empty(n_out, np.int32)
        hip.check(hip.lib().gl3_forward_batch_sample(self._ctx, _p(t), _p(s), _p(p), _p(w) if w is not None else None, t.size,
                                                     _p(te), _p(tp), _p(co), _p(ids)), self._ctx)
        return ids

    def sample_rows(self, logits, temperature, topp, coins) -> np.ndarray:
        """The batched sampler alone on host logits [n][vocab] (no forward pass) -> sampled ids [n]."""
        lg = np.ascontiguousarray(logits, np.float32)
        assert lg.ndim == 2 and lg.shape[1] == self.cfg.vocab
        n = lg.shape[0]
        te, tp, co = self._per_row(temperature, n), self._per_row(topp, n), self._per_row(coins, n)
        ids = np.empty(n, np.int32)
        hip.check(hip.lib().gl3_sample_rows(self._ctx, _p(lg), n, _p(te), _p(tp), _p(co), _p(ids)), self._ctx)
        return ids

    def _score_args(self, targets, temperature, n):
        """targets int32[n] (None: NULL, which the library refuses), temperature f32[n] or None for 1 everywhere, the result array"""
        tg = np.ascontiguousarray(targets, np.int32) if targets is not None else None
        assert tg is None or tg.shape == (n,)
        te = self._per_row(temperature, n) if temperature is not None else None
        return tg, te, np.zeros(n, SCORE_DTYPE)

    def forward_batch_score(self, tokens, seq_ids, positions, targets, temperature=None, want_logits=None):
        """Mixed batched step + the score of one known token per OUTPUT row on the device (gl3_forward_batch_score) -> (scores, greedy ids
        [n_out]).  scores: structured array [n_out] with fields prob, logit, max, sum; targets: one id per output row; temperature: one
        entry per output row (a scalar broadcasts), None = 1."""
        t, s, p, w, n_out = self._mixed_args(tokens, seq_ids, positions, want_logits)
        tg, te, scores = self._score_args(targets, temperature, n_out)
        ids = np.empty(n_out, np.int32)
        hip.check(hip.lib().gl3_forward_batch_score(self._ctx, _p(t), _p(s), _p(p), _p(w) if w is not None else None, t.size,
                                                    _p(tg) if tg is not None else None, _p(te) if te is not None else None,
                                                    _p(scores) if n_out else None, _p(ids) if n_out else None), self._ctx)
        return scores, ids

    def score_rows(self, logits, targets, temperature=None) -> np.ndarray:
        """The scoring kernel alone on host logits [n][vocab] (no forward pass) -> scores [n] (fields prob, logit, max, sum)."""
        lg = np.ascontiguousarray(logits, np.float32)
        assert lg.ndim == 2 and lg.shape[1] == self.cfg.vocab
        n = lg.shape[0]
        tg, te, scores = self._score_args(targets, temperature, n)
        hip.check(hip.lib().gl3_score_rows(self._ctx, _p(lg), n, _p(tg) if tg is not None else None, _p(te) if te is not None else None,
                                           _p(scores)), self._ctx)
        return scores

    @staticmethod
    def _verify_args(temperature, coins, n_runs, n):
        """temperature f32[n_runs] (a scalar broadcasts) or None = greedy everywhere, coins f32[n][2] or None"""
        te = HipMasterPlan._per_row(temperature, n_runs) if temperature is not None else None
        co = np.ascontiguousarray(coins, np.float32) if coins is not None else None
        assert co is None or co.shape == (n, 2)
        return te, co

    def forward_batch_verify(self, tokens, seq_ids, positions, temperature=None, coins=None) -> np.ndarray:
        """Mixed batched step over runs [last real token, drafts ...] + the decision on the device how many drafts of every run stand
        (gl3_forward_batch_verify) -> structured array [n_runs] with fields accepted and token.  temperature: one entry per run (a scalar
        broadcasts), None = greedy everywhere; coins [n][2]: the accept and the emit coin of every row, None when every run is greedy."""
        t, s, p, _, n_runs = self._mixed_args(tokens, seq_ids, positions, None)
        te, co = self._verify_args(temperature, coins, n_runs, t.size)
        res = np.zeros(max(t.size, 1), VERIFY_DTYPE)
        got = C.c_int32(0)
        hip.check(hip.lib().gl3_forward_batch_verify(self._ctx, _p(t), _p(s), _p(p), t.size, _p(te) if te is not None else None,
                                                     _p(co) if co is not None else None, _p(res), C.byref(got)), self._ctx)
        return res[:got.value].copy()

    def verify_rows(self, logits, tokens, run_rows, temperature=None, coins=None) -> np.ndarray:
        """The verification kernel alone on host logits [n][vocab] (no forward pass); run_rows: the rows of every run, summing to n ->
        structured array [n_runs] with fields accepted and token."""
        lg = np.ascontiguousarray(logits, np.float32)
        assert lg.ndim == 2 and lg.shape[1] == self.cfg.vocab
        t = np.ascontiguousarray(tokens, np.int32); rr = np.ascontiguousarray(run_rows, np.int32)
        assert t.size == lg.shape[0] == int(rr.sum())      # the C entry takes its row count from run_rows: it cannot see a mismatch
        te, co = self._verify_args(temperature, coins, rr.size, t.size)
        res = np.zeros(rr.size, VERIFY_DTYPE)
        hip.check(hip.lib().gl3_verify_rows(self._ctx, _p(lg), _p(t), _p(rr), rr.size, _p(te) if te is not None else None,
                                            _p(co) if co is not None else None, _p(res)), self._ctx)
        return res

    def draft_probs_put(self, slot: int, draft_plan: "HipMasterPlan"):
        """Slot `slot` of this (target) plan's draft table = the row draft_plan.sample_probs() returns, copied on the device
        (gl3_draft_probs_put)."""
        hip.check(hip.lib().gl3_draft_probs_put(self._ctx, slot, draft_plan._ctx if draft_plan is not None else None), self._ctx)

    def draft_probs_put_row(self, slot: int, draft_plan: "HipMasterPlan", row: int):
        """Slot `slot` of this (target) plan's draft table = sample_probs_row(row) of draft_plan's last batched sampled step, copied on the
        device (gl3_draft_probs_put_row)."""
        hip.check(hip.lib().gl3_draft_probs_put_row(self._ctx, slot, draft_plan._ctx if draft_plan is not None else None, row), self._ctx)

    def draft_probs_put_host(self, slot: int, q):
        """The same slot from host memory, f32[vocab], taken as it is."""
        q = np.ascontiguousarray(q, np.float32) if q is not None else None
        assert q is None or q.shape == (self.cfg.vocab,)
        hip.check(hip.lib().gl3_draft_probs_put_host(self._ctx, slot, _p(q) if q is not None else None), self._ctx)

    def draft_probs(self, slot: int) -> np.ndarray:
        """Slot `slot` of the draft table back on the host."""
        out = np.empty(self.cfg.vocab, np.float32)
        hip.check(hip.lib().gl3_get_draft_probs(self._ctx, slot, _p(out)), self._ctx)
        return out

    @staticmethod
    def _q_slots(q_slots, n):
        """q_slots int32[n] (a scalar broadcasts; None: NULL, which the library refuses)"""
        return np.ascontiguousarray(np.broadcast_to(np.asarray(q_slots, np.int32), (n,))) if q_slots is not None else None

    def forward_batch_verify_dist(self, tokens, seq_ids, positions, temperature=None, coins=None, q_slots=-1) -> np.ndarray:
        """forward_batch_verify with q_slots: per row the slot of the draft table its draft was drawn from, -1 = a fixed token
        (gl3_forward_batch_verify_dist) -> structured array [n_runs] with fields accepted and token."""
        t, s, p, _, n_runs = self._mixed_args(tokens, seq_ids, positions, None)
        te, co = self._verify_args(temperature, coins, n_runs, t.size)
        qs = self._q_slots(q_slots, t.size)
        res = np.zeros(max(t.size, 1), VERIFY_DTYPE)
        got = C.c_int32(0)
        hip.check(hip.lib().gl3_forward_batch_verify_dist(self._ctx, _p(t), _p(s), _p(p), t.size, _p(te) if te is not None else None,
                                                          _p(co) if co is not None else None, _p(qs) if qs is not None else None,
                                                          _p(res), C.byref(got)), self._ctx)
        return res[:got.value].copy()

    def verify_rows_dist(self, logits, tokens, run_rows, temperature=None, coins=None, q_slots=-1) -> np.ndarray:
        """verify_rows with q_slots (gl3_verify_rows_dist) -> structured array [n_runs] with fields accepted and token."""
        lg = np.ascontiguousarray(logits, np.float32)
        assert lg.ndim == 2 and lg.shape[1] == self.cfg.vocab
        t = np.ascontiguousarray(tokens, np.int32); rr = np.ascontiguousarray(run_rows, np.int32)
        assert t.size == lg.shape[0] == int(rr.sum())
        te, co = self._verify_args(temperature, coins, rr.size, t.size)
        qs = self._q_slots(q_slots, t.size)
        res = np.zeros(rr.size, VERIFY_DTYPE)
        hip.check(hip.lib().gl3_verify_rows_dist(self._ctx, _p(lg), _p(t), _p(rr), rr.size, _p(te) if te is not None else None,
                                                 _p(co) if co is not None else None, _p(qs) if qs is not None else None, _p(res)), self._ctx)
        return res

    def sample_probs_row(self, row: int) -> np.ndarray:
        """The probabilities row `row` of the last batched sampled step was drawn from."""
        out = np.empty(self.cfg.vocab, np.float32)
        hip.check(hip.lib().gl3_get_sample_probs_row(self._ctx, row, _p(out)), self._ctx)
        return out

    def kv_seq(self, seq: int, layer: int, pos: int):
        n = self.cfg.kv_dim // self.tp_size
        k, v = np.empty(n, np.float32), np.empty(n, np.float32)
        hip.check(hip.lib().gl3_get_kv_seq(self._ctx, seq, layer, pos, _p(k), _p(v)), self._ctx)
        return k, v

    def kv_seq_copy(self, src: int, dsts, p0: int, p1: int):
        """Fork a prefix (gl3_kv_seq_copy): the K / V rows [p0, p1) of sequence `src`, every layer, into the same positions of every sequence
        in `dsts`.  Returns after the copy has completed."""
        d = np.ascontiguousarray(dsts, np.int32)
        hip.check(hip.lib().gl3_kv_seq_copy(self._ctx, src, _p(d), d.size, p0, p1), self._ctx)

    def freeTornadoExecutionPlan(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            hip.lib().gl3_destroy(self._ctx)
            self._ctx = C.c_void_p()

    # ---- pythonic conveniences -----------------------------------------------------------------
    def forward_decode(self, token: int, position: int, copy: bool = True):
        hip.check(hip.lib().gl3_forward_decode(self._ctx, token, position, _p(self._logits), None), self._ctx)
        return self._logits.copy() if copy else self._logits

    def forward_decode_argmax(self, token: int, position: int) -> int:
        """-Dllama.deviceSample: greedy token id sampled on the device (4 bytes D2H instead of vocab*4)."""
        hip.check(hip.lib().gl3_forward_decode(self._ctx, token, position, None, C.byref(self._arg)), self._ctx)
        return int(self._arg.value)

    def forward_decode_sample(self, token: int, position: int, temperature: float, topp: float, coin: float) -> int:
        """One decode step + Sampler.selectSampler(...).sampleToken(logits) (Sampler.java:76-123); `coin` = rng.nextFloat(1f) from the
        caller's RandomGenerator (javarand.L32X64MixRandom mirrors RandomGeneratorFactory.getDefault())."""
        out = C.c_int32()
        hip.check(hip.lib().gl3_forward_decode_sample(self._ctx, token, position, temperature, topp, coin, C.byref(out)), self._ctx)
        return int(out.value)

    def forward_decode_chain(self, token: int, position: int, k: int, temperature: float = 0.0, coins=None, target: "HipMasterPlan" = None,
                             slot0: int = 0) -> np.ndarray:
        """k single-token steps behind one wait, each step's id fed to the next on the device (gl3_forward_decode_chain): what k
        forward_decode_sample(t_j, position + j, temperature, 0.0, coins[j]) calls return, int32[k].  temperature 0: a greedy chain, coins
        may be None.  target: every step's probabilities row goes into slot slot0 + j of that plan's draft table, as draft_probs_put."""
        co = np.ascontiguousarray(coins, np.float32) if coins is not None else None
        assert co is None or co.shape == (k,)      # the C entry reads k coins: it cannot see a shorter array
        out = np.zeros(max(k, 1), np.int32)
        hip.check(hip.lib().gl3_forward_decode_chain(self._ctx, token, position, k, temperature, _p(co) if co is not None else None,
                                                     target._ctx if target is not None else None, slot0, _p(out)), self._ctx)
        return out[:k]

    def sample_probs(self) -> np.ndarray:
        out = np.empty(self.cfg.vocab, np.float32)
        hip.check(hip.lib().gl3_get_sample_probs(self._ctx, _p(out)), self._ctx)
        return out

    def prefill(self, tokens, start_pos: int = 0, batch: int | None = None):
        """LlamaBench.prefill (J/bench/LlamaBench.java:258-273): chunks of `batch` (llama-bench -b; default max_batch)."""
        tokens = list(tokens)
        b = max(1, min(batch or self.max_batch, max(1, self.max_batch)))
        for off in range(0, len(tokens), b):
            self.tornadoVMForwardBatchPrefill(tokens[off:off + b], start_pos + off)

    def tp_fold_mode(self):
        """(mode, consumer mask) of the tensor-parallel hand-over of this plan's decode step (gl3_tp_fold_mode)."""
        a, b = C.c_int32(), C.c_int32()
        hip.check(hip.lib().gl3_tp_fold_mode(self._ctx, C.byref(a), C.byref(b)), self._ctx)
        return a.value, b.value

    def topp_counts(self):
        """(top-p draws answered on the device, draws answered by the host heap after a tie at the sampled rank)."""
        a, b = C.c_int64(), C.c_int64()
        hip.check(hip.lib().gl3_get_topp_counts(self._ctx, C.byref(a), C.byref(b)), self._ctx)
        return a.value, b.value

    def x(self):
        out = np.empty(self.cfg.dim, np.float32)
        hip.check(hip.lib().gl3_get_x(self._ctx, _p(out)), self._ctx)
        return out

    def attn_rows(self):
        """Rows of the last batched step by the attention form that served them (gl3_get_attn_rows): [attn_head_kernel, one-launch tiled
        kernels, long-context trio, per-row pair]."""
        out = np.zeros(4, np.int32)
        hip.check(hip.lib().gl3_get_attn_rows(self._ctx, _p(out)), self._ctx)
        return out.tolist()

    def layer_x(self, layer: int):
        out = np.empty(self.cfg.dim, np.float32)
        hip.check(hip.lib().gl3_get_layer_x(self._ctx, layer, _p(out)), self._ctx)
        return out

    def kv(self, layer: int, pos: int):
        n = self.cfg.kv_dim // self.tp_size
        k, v = np.empty(n, np.float32), np.empty(n, np.float32)
        hip.check(hip.lib().gl3_get_kv(self._ctx, layer, pos, _p(k), _p(v)), self._ctx)
        return k, v

    def buffer(self, which: int, n: int):
        out = np.empty(n, np.float32)
        hip.check(hip.lib().gl3_get_buffer(self._ctx, which, _p(out), n), self._ctx)
        return out

    def reset_kv(self):
        hip.check(hip.lib().gl3_reset_kv(self._ctx), self._ctx)

    def profile_decode(self, token: int, position: int) -> dict:
        kt = hip.KernelTimes()
        hip.check(hip.lib().gl3_profile_decode(self._ctx, token, position, C.byref(kt)), self._ctx)
        return {n: dict(ms=kt.ms[i], launches=kt.launches[i], bytes=kt.bytes[i]) for i, n in enumerate(hip.K_NAMES)}

    def profile_kernel(self, klass: str, iters: int = 10) -> dict:
        """One kernel class, back-to-back over every layer's weights, one HIP event pair (see gl3_profile_kernel)."""
        us, nb = C.c_double(), C.c_uint64()
        hip.check(hip.lib().gl3_profile_kernel(self._ctx, hip.K_NAMES.index(klass), iters, C.byref(us), C.byref(nb)), self._ctx)
        return dict(avg_us=us.value, bytes_per_launch=nb.value, gbs=nb.value / us.value / 1e3)

    def profile_prefill_kernel(self, klass: str, n_tokens: int, iters: int = 3) -> dict:
        """One batched-prefill GEMM class at n_tokens tokens (see gl3_profile_prefill_kernel): device time and int8 TOP/s."""
        us, ops = C.c_double(), C.c_uint64()
        hip.check(hip.lib().gl3_profile_prefill_kernel(self._ctx, hip.K_NAMES.index(klass), n_tokens, iters, C.byref(us), C.byref(ops)), self._ctx)
        return dict(avg_us=us.value, int8_ops_per_launch=ops.value, tops=ops.value / us.value / 1e6)

    def init_ms(self):
        a, b = C.c_double(), C.c_double()
        hip.check(hip.lib().gl3_get_init_ms(self._ctx, C.byref(a), C.byref(b)), self._ctx)
        return dict(plan_creation_ms=a.value, weights_copy_in_ms=b.value)

    def __del__(self):
        try:
            self.freeTornadoExecutionPlan()
        except Exception:
            pass


def vl_gemm_plan(weight_type: int, flags: int, rows: int, ntok: int) -> dict:
    """The library's choice for one batched GEMM of the f32-activation weight types (gl3_debug_vl_gemm_plan; no plan, no device):
    kernel name, row tiles, token tiles, grid, and for gemm_vlq_mfma_kernel the tile mapping and vqm_groups' G / P."""
    out = np.zeros(7, np.int32)
    hip.check(hip.lib().gl3_debug_vl_gemm_plan(weight_type, flags, rows, ntok, _p(out)))
    k, nrt, ntt, grid, xcd, g, p = out.tolist()
    return dict(kernel=hip.VL_GEMM_KERNELS[k], nrt=nrt, ntt=ntt, grid=grid, xcd_tokens=xcd, G=g, P=p)


def gemm3_plan(epi: str, rows: int, ntok: int) -> dict:
    """The library's choice for one > 64-token Q8_0 GEMM (gl3_debug_gemm3_plan; no plan, no device).  epi: "store" | "resid" | "swiglu"
    (rows = hidden).  Kernel name, workgroup tile (rows per matrix x tokens), blocks per K stage, NFR of the tall tiling, row and token
    tiles, grid, and whether gate + up writes hb quantised."""
    out = np.zeros(9, np.int32)
    hip.check(hip.lib().gl3_debug_gemm3_plan(hip.GEMM3_EPI[epi], rows, ntok, _p(out)))
    k, tr, tt, kb, nfr, nrt, ntt, grid, qout = out.tolist()
    return dict(kernel=hip.GEMM3_KERNELS[k], tile_rows=tr, tile_tok=tt, KB=kb, NFR=nfr, nrt=nrt, ntt=ntt, grid=grid, qout=qout)


def bd_gemm_plan(epi: str, rows: int, k: int, ntok: int, quantised_out: bool = False, wg: int = -1) -> dict:
    """The library's launch of one Q8_0 GEMM of a step of at most 64 rows (gl3_debug_bd_gemm_plan; no plan, no device).  epi: "store" |
    "resid" | "swiglu" (rows = hidden).  Token slots (0: more than 64 tokens, not this kernel), DA, the quantising form, threads, token
    tiles, units, grid, K tiles / full trips / tiles of the partial trip, and `place`: (unit, token tile) of workgroup wg, None when it
    exits or wg is outside the grid."""
    out = np.zeros(12, np.int32)
    hip.check(hip.lib().gl3_debug_bd_gemm_plan(hip.GEMM3_EPI[epi], rows, k, ntok, int(quantised_out), wg, _p(out)))
    ts, da, qout, threads, ntt, units, grid, ntiles, trips, partial, unit, h = out.tolist()
    return dict(ts=ts, DA=da, qout=qout, threads=threads, ntt=ntt, units=units, grid=grid, ntiles=ntiles, trips=trips, partial=partial,
                place=None if unit < 0 else (unit, h))


def matvec_plan(weight_type: int, flags: int, pro: str, epi: str, rows: int, k: int) -> dict:
    """The library's launch of one decode projection of the f32-activation weight types (gl3_debug_matvec_plan; no plan, no device).
    pro: "rms" | "quant"; epi: "store" | "resid" | "swiglu" (rows = hidden).  Kernel name, whether rmsnorm_f32_kernel runs in front,
    wavefronts per workgroup, MAXW, grid, threads, dynamic LDS bytes and their cap, and matvec_vlq_kernel's nch / nrounds / rc / RCM."""
    out = np.zeros(12, np.int32)
    hip.check(hip.lib().gl3_debug_matvec_plan(weight_type, flags, hip.MATVEC_PRO[pro], hip.GEMM3_EPI[epi], rows, k, _p(out)))
    kern, rms, nw, maxw, grid, threads, lds, cap, nch, nrounds, rc, rcm = out.tolist()
    return dict(kernel=hip.MATVEC_KERNELS[kern], rms_launch=rms, nw=nw, MAXW=maxw, grid=grid, threads=threads, lds=lds, lds_cap=cap,
                nch=nch, nrounds=nrounds, rc=rc, RCM=rcm)


def make_local_group(n: int):
    """Test transport: n plans in one process on one GPU (one host thread per rank)."""
    g = C.c_void_p()
    hip.check(hip.lib().gl3_local_group_create(n, C.byref(g)))
    return g


def make_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    hip.check(hip.lib().gl3_tp_unique_id(buf, 128))
    return buf.raw
