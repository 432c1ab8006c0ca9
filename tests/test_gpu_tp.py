"""Tensor parallelism on ONE GPU: the in-process test transport (gl3_local_group: one host thread per rank,
device-to-device copies instead of RCCL) runs the real row-split plans — same upload slicing, same kernel arguments,
same gather points — and every rank must return logits bit-identical to the single-GPU CPU oracle.
A one-rank RCCL communicator additionally exercises ncclCommInitRank / ncclAllGather inside the library."""
import threading

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


@pytest.mark.parametrize("cfg,tp,wtype", [("mid-llama", 2, 8), ("mid-llama", 4, 8), ("mid-qwen3", 2, 8), ("tiny-llama-tied", 2, 8),
                                          ("mid-llama", 2, 2), ("mid-llama", 4, 1), ("mid-qwen3", 2, 1), ("mid-qwen2", 2, 8),
                                          ("mid-llama", 8, 8), ("mid-llama", 8, 2), ("mid-qwen3", 8, 8), ("mid-granite", 2, 8), ("mid-phi3", 2, 8), ("mid-phi3", 4, 2),
                                          ("tiny-llama-tied", 4, 2)])    # vocab / tp = 160: whole 8-row groups, not a multiple of 64 (Llama-3's 128256 / 8 = 16032)   # BASELINE configs[3]: Q4_0 row split, tp = 8 (one kv head per rank)
def test_row_split_ranks_are_bit_identical_to_the_oracle(pkg, orc, planmod, cfg, tp, wtype):
    if tp >= 4:
        # four or more polling ranks need one hardware queue per rank stream; late in a long-lived process the runtime multiplexes streams onto shared
        # queues (tests/conftest.py: seen as a gather time-out in the 10th group of a process), so these groups run in a fresh process each
        import os, subprocess, sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        r = subprocess.run([sys.executable, os.path.join(root, "scripts", "debug_tp_fold.py"), cfg, str(tp), "2", str(wtype)], cwd=root,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return
    plan_mod, hip = planmod
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], wtype=wtype, seed=17)
    o = orc.COracle(m, vector_bits=0 if wtype == 8 else 256)         # F16 / Q4_0: the plan's default Vector-API dot order
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, 4 if tp <= 2 else 2)     # in-process ranks time-share one GPU: keep tp >= 4 short
    ref = [o.forward(t, p) for p, t in enumerate(toks)]
    grp = plan_mod.make_local_group(tp)
    out = [None] * tp
    err = [None] * tp

    def rank_main(r):
        try:
            plan = plan_mod.HipMasterPlan(m, tp_rank=r, tp_size=tp, local_group=grp)
            out[r] = [plan.forward_decode(t, p) for p, t in enumerate(toks)]
            plan.freeTornadoExecutionPlan()
        except Exception as e:   # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(tp)]
    [t.start() for t in th]
    [t.join(timeout=900) for t in th]
    assert all(e is None for e in err), err
    assert not any(t.is_alive() for t in th)
    hip.lib().gl3_local_group_destroy(grp)
    for r in range(tp):
        for p in range(len(toks)):
            assert np.array_equal(out[r][p], ref[p]), (r, p)


def test_row_split_ranks_on_edge_values(pkg, orc, planmod):
    """tp = 2 on the "all" model of tests/edge_models.py (tiny-llama-tied, Q8_0): the row-split upload slicing and the folded gathers see
    -128 quants, zero / subnormal / negative / 2^15 block scales and zero, subnormal-scaled and outlier activation blocks; every rank's
    logits equal the oracle's bit for bit."""
    import edge_models as em
    plan_mod, hip = planmod
    m = em.make_edge_model("tiny-llama-tied", 8, 7, "all")
    o = orc.COracle(m)
    toks = em.edge_tokens(pkg, m, 8)
    ref = [o.forward(t, p) for p, t in enumerate(toks)]
    assert all(np.all(np.isfinite(r)) for r in ref)
    grp = plan_mod.make_local_group(2)
    out, err = [None] * 2, [None] * 2

    def rank_main(r):
        try:
            plan = plan_mod.HipMasterPlan(m, tp_rank=r, tp_size=2, local_group=grp)
            out[r] = [plan.forward_decode(t, p) for p, t in enumerate(toks)]
            plan.freeTornadoExecutionPlan()
        except Exception as e:   # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
    [t.start() for t in th]
    [t.join(timeout=900) for t in th]
    assert all(e is None for e in err), err
    assert not any(t.is_alive() for t in th)
    hip.lib().gl3_local_group_destroy(grp)
    for r in range(2):
        for p in range(len(toks)):
            assert np.array_equal(out[r][p], ref[p]), (r, p)


def test_q8_decode_gathers_are_folded_into_the_producers(pkg, orc, planmod):
    """The default hand-over of the decode step: the attention / gate-up / down kernels write their results into the peers' arenas (mode 1) — the
    Q8_0 int8 path and, since r6, the vector-order F16 / Q4_0 plans (BASELINE configs[3] is Q4_0 TP = 8); the scalar-order kernels
    (GL3_FLAG_SCALAR_DOT) keep the gather launches (mode 0).  (Bit-exactness of all of them: the row-split test above.)"""
    plan_mod, hip = planmod
    for wtype, flags, want in ((8, 0, 1), (2, 0, 1), (1, 0, 1), (2, hip.FLAG_SCALAR_DOT, 0)):
        m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], wtype=wtype, seed=3)
        grp = plan_mod.make_local_group(2)
        modes, err = [None, None], [None, None]

        def rank_main(r):
            try:
                plan = plan_mod.HipMasterPlan(m, tp_rank=r, tp_size=2, local_group=grp, flags=flags)
                modes[r] = plan.tp_fold_mode()
                plan.forward_decode(1, 0)
                plan.freeTornadoExecutionPlan()
            except Exception as e:   # noqa: BLE001
                err[r] = e
        th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
        [t.start() for t in th]; [t.join(timeout=300) for t in th]
        hip.lib().gl3_local_group_destroy(grp)
        assert err == [None, None], err
        assert modes == [(want, 0), (want, 0)], (wtype, flags, modes)


@pytest.mark.parametrize("cfg,tp,mask,wgs", [("mid-llama", 4, None, 16), ("mid-qwen3", 8, None, 16), ("mid-llama", 2, "5", 16), ("mid-llama", 2, None, 256)])
def test_gathers_folded_into_the_consumer_prologues(cfg, tp, mask, wgs):
    """GL3_TP_FOLD=2: no launch between producer and consumer — wo / down / qkv / logits / the embedding wait for the peers in their own
    prologue.  A consumer that polls holds its compute units, so ranks that SHARE one GPU (this test) must leave room for each other's
    producers: GL3_WGS=16 caps every matvec at 16 workgroups (with full grids four ranks' wo launches fill the chip and the laggard's
    attention kernel never starts — seen as a gather time-out, not a wrong result).  Separate process: the switches are read at plan
    creation / first launch.  The third case mixes prologue waits (wo, qkv) with wait launches (GL3_TP_FOLD_MASK); the fourth runs two ranks at the
    production launch geometry of one workgroup per CU and rank (GL3_WGS=256: both ranks' polling consumers and producers fit the chip together)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GL3_TP_FOLD="2", GL3_WGS=str(wgs))
    if mask: env["GL3_TP_FOLD_MASK"] = mask
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "debug_tp_fold.py"), cfg, str(tp), "3"], env=env, cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert ("fold mode 1 mask %s" % (mask or "31")) in r.stdout, r.stdout[-1000:]


def test_single_rank_rccl_communicator(pkg, orc, planmod):
    plan_mod, hip = planmod
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=7)
    o = orc.COracle(m)
    uid = plan_mod.make_unique_id()
    plan = plan_mod.HipMasterPlan(m, flags=hip.FLAG_FORCE_RCCL, unique_id=uid)      # tp_size = 1, all-gathers still issued
    for pos, t in enumerate(pkg.javarand.bench_tokens(m.cfg.vocab, 4)):
        assert np.array_equal(plan.forward_decode(t, pos), o.forward(t, pos))
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("cfg,tp,chunks,wtype,f32act", [("mid-llama", 2, [40, 9], 8, False), ("mid-qwen3", 2, [20, 7], 8, False),
                                                       ("mid-llama", 2, [40, 9], 1, False), ("mid-granite", 4, [40, 9], 1, False),
                                                       # r5: the VALU GEMM types are back in the in-process group.  Round 4 saw single wrong activation rows here in
                                                       # ~1 of 3 runs; root cause (profiles/r05_tp_flake.md): a freed hipDeviceMallocUncached arena was recycled by
                                                       # the HIP allocator under the cached policy for the NEXT plans of the same process — fixed by the process-wide
                                                       # arena pool in gl3_tp.hip (100 of 100 clean loops; 9 of 10 failing with GL3_TP_ARENA=unpooled)
                                                       ("mid-llama", 4, [33, 20], 2, False), ("mid-llama", 2, [50, 9], 8, True), ("mid-llama", 2, [33, 20], 2, False)])
def test_batched_prefill_under_row_split(pkg, orc, planmod, cfg, tp, chunks, wtype, f32act):
    """Batched prefill on tensor-parallel ranks (int8 MFMA for Q8_0; gl3_prefill_vl.h for F16 / Q4_0 / Q8_0 with the f32 activation):
    row-split GEMMs, rank-chunked activations, three all-gathers per layer.  Every rank's KV slice and the decode steps that
    follow must equal the CPU oracle bit for bit."""
    plan_mod, hip = planmod
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], wtype=wtype, seed=41)
    o = orc.COracle(m, vector_bits=0 if (wtype == 8 and not f32act) else 256, f32_activation=f32act)
    flags = hip.FLAG_F32_ACTIVATION if f32act else 0
    n = sum(chunks)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, n + 2)
    o.prefill(toks[:n], 0)
    ref = [o.forward(toks[n], n), o.forward(toks[n + 1], n + 1)]
    kvl = m.cfg.kv_dim // tp
    grp = plan_mod.make_local_group(tp)
    out, kvs, err = [None] * tp, [None] * tp, [None] * tp

    def rank_main(r):
        try:
            plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, tp_rank=r, tp_size=tp, local_group=grp, flags=flags)
            pos = 0
            for c in chunks:
                plan.tornadoVMForwardBatchPrefill(toks[pos:pos + c], pos)
                pos += c
            out[r] = [plan.forward_decode(toks[n], n), plan.forward_decode(toks[n + 1], n + 1)]
            kvs[r] = [plan.kv(l, p) for l in range(m.cfg.n_layers) for p in (0, n // 2, n - 1)]
            plan.freeTornadoExecutionPlan()
        except Exception as e:   # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(tp)]
    [t.start() for t in th]
    [t.join(timeout=900) for t in th]
    assert all(e is None for e in err), err
    assert not any(t.is_alive() for t in th)
    hip.lib().gl3_local_group_destroy(grp)
    for r in range(tp):
        assert np.array_equal(out[r][0], ref[0]) and np.array_equal(out[r][1], ref[1]), r
        i = 0
        for l in range(m.cfg.n_layers):
            for p in (0, n // 2, n - 1):
                ko, vo = o.kv(l, p)
                k, v = kvs[r][i]; i += 1
                assert np.array_equal(k, ko[r * kvl:(r + 1) * kvl]) and np.array_equal(v, vo[r * kvl:(r + 1) * kvl]), (r, l, p)


@pytest.mark.parametrize("wtype", [8, 1, 2])
def test_static_batched_decode_under_row_split(pkg, orc, planmod, wtype):
    """BASELINE configs[4] on tensor-parallel ranks: vocab rows are split, the per-rank logits chunks are gathered in place and
    un-chunked on the way to the host; logits and greedy ids of every sequence equal the oracle's on every rank (Q8_0, and r4:
    Q4_0 / F16 in the Vector-API order)."""
    plan_mod, hip = planmod
    tp, nseq, steps = 2, 3, 3
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["mid-llama"], wtype=wtype, seed=43)
    toks = np.asarray(pkg.javarand.bench_tokens(m.cfg.vocab, nseq * steps), np.int32).reshape(steps, nseq)
    ref = []
    for s in range(nseq):
        o = orc.COracle(m, vector_bits=0 if wtype == 8 else 256)
        ref.append([o.forward(int(toks[i, s]), i) for i in range(steps)])
    grp = plan_mod.make_local_group(tp)
    out, err = [None] * tp, [None] * tp

    def rank_main(r):
        try:
            plan = plan_mod.HipMasterPlan(m, prefill_batch_size=8, n_seqs=nseq, tp_rank=r, tp_size=tp, local_group=grp)
            res = []
            for i in range(steps):
                lg, ids = plan.forward_decode_batch(toks[i], np.arange(nseq, dtype=np.int32), np.full(nseq, i, np.int32))
                res.append((lg.copy(), ids.copy()))
            out[r] = res
            plan.freeTornadoExecutionPlan()
        except Exception as e:   # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(tp)]
    [t.start() for t in th]
    [t.join(timeout=900) for t in th]
    assert all(e is None for e in err), err
    assert not any(t.is_alive() for t in th)
    hip.lib().gl3_local_group_destroy(grp)
    for r in range(tp):
        for i in range(steps):
            lg, ids = out[r][i]
            for s in range(nseq):
                assert np.array_equal(lg[s], ref[s][i]), (r, i, s)
                assert int(ids[s]) == orc.argmax(ref[s][i])


def test_static_batched_decode_under_row_split_at_mixed_depths_across_128(pkg, orc, planmod):
    """The same step on two row-split ranks with the rows at different depths on both sides of position 128 (sequences prefilled to 126, 4
    and 129 positions, in chunks of 64): the three-kernel attention on this rank's heads reads every row's own sequence and position, the
    attention output / hb go through the gathers and the separate quantise launches, every step is enqueued eagerly; sequence 0 walks
    127 -> 128.  Logits and greedy ids of every row equal its own oracle's on both ranks, in changing row order, and so does each rank's
    slice of the K / V rows the steps wrote in every sequence's cache."""
    plan_mod, hip = planmod
    tp, lens, steps = 2, [126, 4, 129], 4
    nseq = len(lens)
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["mid-llama"], wtype=8, seed=47)
    assert m.cfg.ctx > max(lens) + steps
    rng = np.random.default_rng(7)
    prompts = [rng.integers(0, m.cfg.vocab, n).tolist() for n in lens]
    first = [int(rng.integers(0, m.cfg.vocab)) for _ in lens]
    orders = [[0, 1, 2], [2, 0, 1], [1, 2, 0], [2, 1, 0]]
    ref, ref_kv = [], {}                                      # ref[s][i]: logits of sequence s at step i, greedy continuation
    for s in range(nseq):
        o = orc.COracle(m)
        o.prefill(prompts[s], 0)
        t, rows = first[s], []
        for i in range(steps):
            rows.append(o.forward(t, lens[s] + i))
            t = orc.argmax(rows[-1])
        ref.append(rows)
        for l in range(m.cfg.n_layers):
            for p in range(lens[s] - 1, lens[s] + steps + 1):
                ref_kv[(s, l, p)] = o.kv(l, p)
    assert lens[0] + 1 == 127 and lens[0] + steps - 1 >= 128 and max(lens) >= 128 > min(lens) + steps
    grp = plan_mod.make_local_group(tp)
    out, kvs, err = [None] * tp, [None] * tp, [None] * tp

    def rank_main(r):
        try:
            plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=nseq, tp_rank=r, tp_size=tp, local_group=grp)
            for s in range(nseq):
                plan.prefill_seq(s, prompts[s], 0)
            cur, res = list(first), []
            for i in range(steps):
                order = orders[i]
                lg, ids = plan.forward_decode_batch([cur[s] for s in order], order, [lens[s] + i for s in order])
                res.append((lg.copy(), ids.copy()))
                for row, s in enumerate(order):
                    cur[s] = int(ids[row])
            out[r] = res
            # this rank's slice of every K / V row the steps wrote, one before and one after (unwritten: zeros on both sides)
            kvs[r] = {(s, l, p): plan.kv_seq(s, l, p) for s in range(nseq) for l in range(m.cfg.n_layers) for p in range(lens[s] - 1, lens[s] + steps + 1)}
            plan.freeTornadoExecutionPlan()
        except Exception as e:   # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(tp)]
    [t.start() for t in th]
    [t.join(timeout=900) for t in th]
    assert all(e is None for e in err), err
    assert not any(t.is_alive() for t in th)
    hip.lib().gl3_local_group_destroy(grp)
    for r in range(tp):
        for i in range(steps):
            lg, ids = out[r][i]
            for row, s in enumerate(orders[i]):
                assert np.array_equal(lg[row], ref[s][i]), (r, i, row, s)
                assert int(ids[row]) == orc.argmax(ref[s][i]), (r, i, row, s)
        kvl = m.cfg.kv_dim // tp
        for key, (ko, vo) in ref_kv.items():
            k, v = kvs[r][key]
            assert np.array_equal(k, ko[r * kvl:(r + 1) * kvl]) and np.array_equal(v, vo[r * kvl:(r + 1) * kvl]), (r,) + key


# ---------------------------------------------------------------------------------------------------------------------
# The production transport between PROCESSES: every rank exports the IPC handle of its arena, the handles travel over
# torch.distributed (gloo), peers are mapped with hipIpcOpenMemHandle and the gather kernel stores into them.  On the
# one-GPU test box all ranks share device 0 (on the 8-GPU node the same code path maps the peers over xGMI).
def _p2p_worker(rank, world, port, cfg_name, wtype, q, f32act=False):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch  # noqa: F401
    import torch.distributed as dist
    import __graft_entry__ as ge
    from importlib import import_module
    pkg = ge.load_package()
    plan_mod = import_module(ge.PKG_NAME + ".plan")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def exchange(handle):
        out = [None] * world
        dist.all_gather_object(out, handle)
        return out

    m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg_name], wtype=wtype, seed=17)
    hip = import_module(ge.PKG_NAME + ".hip")
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, tp_rank=rank, tp_size=world, p2p_exchange=exchange,
                                  flags=hip.FLAG_F32_ACTIVATION if f32act else 0)      # batched prefill for every type (r4)
    dist.barrier()
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, 44)
    plan.prefill(toks[:37], 0)                                    # batched prefill under TP: chunks of 16, 16, 5
    out = [plan.forward_decode(toks[p], p) for p in range(37, 44)]
    ids = [plan.forward_decode_argmax(toks[43], 43)]
    dist.barrier()                                                # nobody unmaps an arena a peer may still be writing
    plan.freeTornadoExecutionPlan()
    q.put((rank, out, ids))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("cfg,world,wtype,f32act", [("mid-llama", 2, 8, False), ("mid-llama", 4, 2, False), ("mid-llama", 2, 1, False), ("mid-llama", 2, 8, True)])
def test_peer_write_transport_between_processes(pkg, orc, cfg, world, wtype, f32act):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_p2p_worker, args=(r, world, port, cfg, wtype, q, f32act)) for r in range(world)]
    [p.start() for p in procs]
    got = {}
    for _ in range(world):
        r, out, ids = q.get(timeout=600)
        got[r] = (out, ids)
    [p.join(timeout=120) for p in procs]
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], wtype=wtype, seed=17)
    modes = dict(vector_bits=0 if (wtype == 8 and not f32act) else 256, f32_activation=f32act)
    o = orc.COracle(m, **modes)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, 44)
    o.prefill(toks[:37], 0)
    ref = [o.forward(toks[p], p) for p in range(37, 44)]
    for r in range(world):
        for i in range(7):
            assert np.array_equal(got[r][0][i], ref[i]), (r, i)
        assert got[r][1][0] == orc.argmax(ref[6])


# ---------------------------------------------------------------------------------------------------------------------
# Row-split ranks at depth: the decode attention regimes behind position 128 and 768 (whose kernels hand xb to the peers themselves under folded
# gathers), prefill chunks that start deep in the context, and the prefix fork.  Schedules and what each is meant to run: tests/tp_depth.py,
# checked against the library's plan without a GPU by tests/test_attn_shapes.py.
def run_ranks(planmod, tp, make_plan, body, env=None, timeout=300):
    """Start tp rank threads, join them within `timeout` seconds in all, collect results and errors, destroy the group.  Rank r creates its plan
    with make_plan(r, group), meets the others (and this thread) at a host-level barrier and returns body(r, plan); its plan is freed behind it.
    `env` is set in os.environ only while the plans are being created (the switches are read in gl3_create / gl3_finalize).  -> [result of rank r]"""
    import os, time
    plan_mod, hip = planmod
    grp = plan_mod.make_local_group(tp)
    out, err = [None] * tp, [None] * tp
    created = threading.Barrier(tp + 1)

    def rank_main(r):
        plan = None
        try:
            try:
                plan = make_plan(r, grp)
            except BaseException:
                created.abort()
                raise
            created.wait()
            created.wait()                                        # ... and goes on once the environment is back as it was
            out[r] = body(r, plan)
        except Exception as e:   # noqa: BLE001
            err[r] = e
        finally:
            if plan is not None:
                plan.freeTornadoExecutionPlan()

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(tp)]
    deadline = time.monotonic() + timeout
    saved = {k: os.environ.get(k) for k in (env or {})}

    def meet():
        try:
            created.wait(max(0.0, deadline - time.monotonic()))
        except threading.BrokenBarrierError:
            pass                                                  # a rank failed to create its plan (err says why), or one did not arrive in time

    os.environ.update(env or {})
    try:
        [t.start() for t in th]
        meet()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    meet()
    [t.join(timeout=max(0.0, deadline - time.monotonic())) for t in th]
    assert not any(t.is_alive() for t in th), "a rank is still running after %d s" % timeout      # (the group stays: that rank still uses it)
    hip.lib().gl3_local_group_destroy(grp)
    assert all(e is None for e in err), err
    return out


def model_at(pkg, cfg, ctx, wtype, seed):
    base = pkg.synth.CONFIGS[cfg]
    return pkg.synth.make_numpy(pkg.synth.ModelConfig(**{**base.__dict__, "ctx": ctx}), wtype=wtype, seed=seed)


def kv_slices_equal(got, want, r, kvl):
    (k, v), (ko, vo) = got, want
    return np.array_equal(k, ko[r * kvl:(r + 1) * kvl]) and np.array_equal(v, vo[r * kvl:(r + 1) * kvl])


_depth_refs = {}


def depth_reference(pkg, orc, cfg, wtype, schedule):
    """(model, tokens by position, {position: oracle logits}, {(layer, row): oracle K / V}) of a schedule; computed once per model and schedule"""
    import tp_depth as td
    key = (cfg, wtype, schedule)
    if key not in _depth_refs:
        m = model_at(pkg, cfg, schedule.ctx, wtype, seed=17)
        o = orc.COracle(m, vector_bits=0 if wtype == 8 else 256)
        toks = pkg.javarand.bench_tokens(m.cfg.vocab, schedule.ctx)
        if schedule.prefill:
            o.prefill(toks[:schedule.prefill], 0)
        logits = {p: o.forward(toks[p], p) for p in td.positions(schedule)}
        kv = {(l, p): o.kv(l, p) for l in range(m.cfg.n_layers) for p in td.kv_rows(schedule)}
        assert all(ko.any() and vo.any() for ko, vo in kv.values())
        _depth_refs[key] = (m, toks, logits, kv)
    return _depth_refs[key]


@pytest.mark.parametrize("name", ["tiny-llama-q8", "mid-llama-q8", "mid-qwen3-q8", "mid-qwen2-q8", "mid-llama-q4", "mid-llama-f16", "mid-llama-q8-eager",
                                  "mid-llama-q8-tp4", "tiny-llama-nofused", "tiny-llama-window", "tiny-llama-mid0", "tiny-llama-gather"])
def test_decode_attention_regimes_on_row_split_ranks(pkg, orc, planmod, name):
    """A rank's decode steps on both sides of positions 128, 768 and 1024 (tests/tp_depth.py): with folded gathers the last attention kernel of a
    step — attn_head_kernel below 128, attn_softmax_pv_kernel up to 767, attn_pv_kernel from 768 — stores xb into the peers' arenas and publishes
    the flag, and the step goes from one regime's captured graph to the next with the step word and the ticket counters live.  Every rank's logits
    at every step, its greedy id at the end of every stretch and its slice of the K / V rows at the hand-overs equal the oracle's; the fold mode
    says which hand-over ran (tiny-llama-gather: the gather launches, as the control)."""
    import tp_depth as td
    plan_mod, hip = planmod
    case = td.CASES[name]
    sched = case.schedule
    if case.child:
        import os, subprocess, sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        r = subprocess.run([sys.executable, os.path.join(root, "scripts", "debug_tp_fold.py"), case.cfg, str(case.tp), "0", str(case.wtype), td.schedule_arg(sched)],
                           env=dict(os.environ, **case.env), cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert ("fold mode %d mask %d" % case.fold) in r.stdout, r.stdout[-1000:]
        return
    m, toks, ref, ref_kv = depth_reference(pkg, orc, case.cfg, case.wtype, sched)

    def make_plan(r, grp):
        return plan_mod.HipMasterPlan(m, prefill_batch_size=sched.batch, tp_rank=r, tp_size=case.tp, local_group=grp, flags=hip.FLAG_NO_GRAPH if case.no_graph else 0)

    def body(r, plan):
        pos = 0
        for c in td.chunks(sched):
            plan.tornadoVMForwardBatchPrefill(toks[pos:pos + c], pos)
            pos += c
        logits = {p: plan.forward_decode(toks[p], p) for p in td.positions(sched)}
        ids = {hi: plan.forward_decode_argmax(toks[hi], hi) for _, hi in sched.stretches}      # the step repeated: it rewrites its K / V row with the same values
        return plan.tp_fold_mode(), logits, ids, {key: plan.kv(*key) for key in ref_kv}

    out = run_ranks(planmod, case.tp, make_plan, body, env=case.env)
    kvl = m.cfg.kv_dim // case.tp
    for r, (mode, logits, ids, kv) in enumerate(out):
        assert mode == case.fold, (r, mode)
        for p in td.positions(sched):
            assert np.array_equal(logits[p], ref[p]), (r, p, td.intended(case, p))
        for _, hi in sched.stretches:
            assert ids[hi] == orc.argmax(ref[hi]), (r, hi)
        for key in ref_kv:
            assert kv_slices_equal(kv[key], ref_kv[key], r, kvl), (r,) + key


@pytest.mark.parametrize("cfg,ctx,batch,chunks,steps", [("tiny-llama", 1300, 512, [512, 512, 76], 4), ("tiny-qwen3", 1300, 512, [512, 512, 76], 4),
                                                        ("mid-llama", 400, 128, [100, 128, 57], 2)])
def test_deep_prefill_chunks_on_row_split_ranks(pkg, orc, planmod, cfg, ctx, batch, chunks, steps):
    """Batched prefill chunks that start deep in the context, on two ranks: chunks of 512, 512 and 76 (the second and third start at 512 and 1024:
    the tiled and long-context prefill attention on the rank's heads_l / kv_heads_l, rank-chunked activations), and on mid-llama (16 query heads per
    rank) chunks of 100, 128 and 57 that straddle 128 and 256.  The decode steps behind them and each rank's K / V slices at the chunk edges
    equal the oracle's."""
    plan_mod, hip = planmod
    tp, n = 2, sum(chunks)
    m = model_at(pkg, cfg, ctx, 8, seed=31)
    o = orc.COracle(m)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, n + steps)
    o.prefill(toks[:n], 0)
    ref = [o.forward(toks[p], p) for p in range(n, n + steps)]
    edges = np.cumsum(chunks).tolist()
    rows = sorted({0, n + steps - 1} | {e - 1 for e in edges} | {e for e in edges[:-1]})
    assert rows == ([0, 511, 512, 1023, 1024, 1099, 1103] if n == 1100 else [0, 99, 100, 227, 228, 284, 286])
    ref_kv = {(l, p): o.kv(l, p) for l in range(m.cfg.n_layers) for p in rows}

    def make_plan(r, grp):
        return plan_mod.HipMasterPlan(m, prefill_batch_size=batch, tp_rank=r, tp_size=tp, local_group=grp)

    def body(r, plan):
        pos = 0
        for c in chunks:
            plan.tornadoVMForwardBatchPrefill(toks[pos:pos + c], pos)
            pos += c
        return [plan.forward_decode(toks[p], p) for p in range(n, n + steps)], {key: plan.kv(*key) for key in ref_kv}

    out = run_ranks(planmod, tp, make_plan, body)
    kvl = m.cfg.kv_dim // tp
    for r, (logits, kv) in enumerate(out):
        for i in range(steps):
            assert np.array_equal(logits[i], ref[i]), (r, n + i)
        for key in ref_kv:
            assert kv_slices_equal(kv[key], ref_kv[key], r, kvl), (r,) + key


def test_prefix_fork_on_row_split_ranks(pkg, orc, planmod):
    """gl3_kv_seq_copy is rank-local under tensor parallelism: every rank copies its own kv_dim / tp slice.  Two ranks prefill sequence 0 with 140
    tokens (chunks of 64, 64, 12), fork rows [0, 140) to sequences 1 and 2 and run three static-batched decode steps in which every sequence
    continues with its own token: logits and greedy ids of every row equal the oracle that was fed that sequence's tokens, the forked rows equal the
    source's and the oracle's slice, the row behind the last step is still zero.  A second fork of rows [64, 100) into the reset plan leaves the
    rows on either side of the range zero."""
    plan_mod, hip = planmod
    tp, nseq, n, steps = 2, 3, 140, 3
    m = model_at(pkg, "tiny-llama", 200, 8, seed=53)
    rng = np.random.default_rng(11)
    prompt = rng.integers(0, m.cfg.vocab, n).tolist()
    first = [int(t) for t in rng.choice(m.cfg.vocab, nseq, replace=False)]
    ref, ref_kv = [], {}
    for s in range(nseq):
        o = orc.COracle(m)
        o.prefill(prompt, 0)
        t, rows = first[s], []
        for i in range(steps):
            rows.append(o.forward(t, n + i))
            t = orc.argmax(rows[-1])
        ref.append(rows)
        for l in range(m.cfg.n_layers):
            for p in (0, 127, 128, n - 1, n, n + steps - 1):
                ref_kv[(s, l, p)] = o.kv(l, p)
    assert not np.array_equal(ref[0][0], ref[1][0]) and not np.array_equal(ref[1][0], ref[2][0])
    forked = [(s, l, p) for s in (1, 2) for l in range(m.cfg.n_layers) for p in (0, 127, 128, n - 1)]
    second = [(l, p) for l in range(m.cfg.n_layers) for p in (63, 64, 99, 100)]

    def make_plan(r, grp):
        return plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=nseq, tp_rank=r, tp_size=tp, local_group=grp)

    def body(r, plan):
        plan.prefill_seq(0, prompt, 0)
        plan.kv_seq_copy(0, [1, 2], 0, n)
        src = {(l, p): plan.kv_seq(0, l, p) for _, l, p in forked}
        cur, res = list(first), []
        for i in range(steps):
            lg, ids = plan.forward_decode_batch(cur, np.arange(nseq, dtype=np.int32), np.full(nseq, n + i, np.int32))
            res.append((lg.copy(), ids.copy()))
            cur = [int(t) for t in ids]
        kv = {key: plan.kv_seq(*key) for key in ref_kv}
        behind = {(s, l): plan.kv_seq(s, l, n + steps) for s in range(nseq) for l in range(m.cfg.n_layers)}
        plan.reset_kv()
        plan.prefill_seq(0, prompt, 0)
        plan.kv_seq_copy(0, [1], 64, 100)
        return res, kv, src, behind, {key: (plan.kv_seq(0, *key), plan.kv_seq(1, *key), plan.kv_seq(2, *key)) for key in second}

    out = run_ranks(planmod, tp, make_plan, body)
    kvl = m.cfg.kv_dim // tp
    for r, (res, kv, src, behind, after) in enumerate(out):
        for i in range(steps):
            lg, ids = res[i]
            for s in range(nseq):
                assert np.array_equal(lg[s], ref[s][i]), (r, i, s)
                assert int(ids[s]) == orc.argmax(ref[s][i]), (r, i, s)
        for key in ref_kv:
            assert kv_slices_equal(kv[key], ref_kv[key], r, kvl), (r,) + key
        for s, l, p in forked:
            assert src[(l, p)][0].any() and src[(l, p)][1].any()
            assert np.array_equal(kv[(s, l, p)][0], src[(l, p)][0]) and np.array_equal(kv[(s, l, p)][1], src[(l, p)][1]), (r, s, l, p)
        assert all(not k.any() and not v.any() for k, v in behind.values()), r
        for (l, p), (s0, s1, s2) in after.items():
            assert s0[0].any() and s0[1].any() and not s2[0].any() and not s2[1].any(), (r, l, p)
            if 64 <= p < 100:
                assert np.array_equal(s1[0], s0[0]) and np.array_equal(s1[1], s0[1]), (r, l, p)
            else:
                assert not s1[0].any() and not s1[1].any(), (r, l, p)
