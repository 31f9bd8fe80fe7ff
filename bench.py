#!/usr/bin/env python3
"""bench.py — 10-iteration bundle adjustment on MI355X.

One "step" = the reference sample's timed region (samples/sample_ba_from_file/main.cpp:185-190):
ONE contiguous `initialize(); optimize(10)` on the kitti_00-shaped synthetic graph (BASELINE.json
configs[1]: 1322 poses / 133 383 landmarks / 561 116 edges, fp64).  The graph lives in host
objects (the API hands over a pointer graph, as the reference's does), so initialize() — flatten +
45 MB of host-to-device copies — is inside the step.  Protocol of the sample: a warm-up
initialize()+optimize(1) on the same optimiser first; unlike the sample the estimates are reset
afterwards, so every step solves the same problem.

  value / ms_per_step      initialize()+optimize(10) on the graph of the warm-up with new estimates:
                           the flattened graph, the Hsc pattern, the ordering and the symbolic
                           factor are re-used (nothing but estimates changed), the reference fork's
                           isDirty idea (src/block_solver.cpp:151-216) carried through
  reflatten                the same region with CUGO_NO_FLATTEN_REUSE=1 (full flattening + 45 MB of
                           host-to-device copies inside the step, structure kept)
  structure_dirty          the same region with CUGO_NO_STRUCTURE_REUSE=1 (pattern + ordering +
                           symbolic analysis rebuilt inside the step)
  optimize_only            optimize(10) alone, inputs resident in HBM (no PCIe in the region)

  python bench.py [--gpus N] [--steps K] [--warmup W] [--workload kitti00|kitti07|synth10k|localba]
                  [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps and prints the result line.  --full adds everything
else: reflatten / structure_dirty / optimize_only, the kernel-timing passes (kernel_groups, kernels,
roofline) and the CPU baseline with its parity check.  --dump-outputs DIR writes what the last timed
step computed (poses, landmarks, chi2 and lambda per LM iteration) as DIR/<name>.npy; the inputs are
seeded, so two builds can be compared output for output.

N > 1 (launched by torch.distributed.run, one rank per GPU): the graph is sharded by landmark
ranges; every LM trial all-reduces [Hsc | bsc] and (F-hat, scale) with RCCL on the solver's stream
INSIDE libcugo_hip.so (cugo_comm_*), the sparse LL^T is replicated — strong scaling on a fixed graph.
"""
import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WORKLOADS = {
    # name: (poses, landmarks, edges, seed, loop-closure landmarks, stereo fraction)
    "kitti00": (1322, 133383, 561116, 0, 4000, 0.7),
    "kitti07": (248, 26127, 95037, 7, 500, 0.7),
    "synth10k": (10000, 1000000, 5000000, 10000, 0, 0.0),
    # ORB-SLAM2-style local BA window (launch-latency regime; not a BASELINE config)
    "localba": (30, 3000, 12600, 30, 0, 0.7),
}
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
FP64_PEAK_TFLOPS = 78.6    # MI355X fp64 vector / matrix peak
PROFILE_ROUND = "r04"
POOL_MAX = 32              # optimisers built for the timed steps; more steps cycle over them


def survey_bytes(group, E, P, L, B):
    """SURVEY.md 8(d) per-unit figures (mono, per-edge information + camera) x units per launch"""
    if group == "build":
        return 249.0 * E + 336.0 * P + 96.0 * L
    if group == "errors":
        return 124.0 * E + 56.0 * P + 24.0 * L
    if group == "schur":
        return (292.0 + 288.0) * E + 172.0 * L + 288.0 * B
    if group == "backsubst_update":
        return 148.0 * E + 120.0 * L + 200.0 * P + 120.0 * L
    return None


def compulsory_bytes(E, Em, Es, P, L, B, f32):
    """Bytes every kernel of THIS layout has to move at least once per launch (its own arrays, each
    touched once; Em / Es = mono / stereo edges).  Never more than the SURVEY 8(d) figure of its
    group; the fraction of a kernel is computed from this count, so it cannot exceed 1."""
    blk = 72.0 if f32 else 144.0   # one 6x3 block of Hpl or T
    meas = 16.0 * Em + 24.0 * Es
    return {
        # idx 8 + meas + omega 8 + flag 1; poses / landmarks once; partial sums are negligible
        "k_errors": 17.0 * E + meas + 56.0 * P + 24.0 * L,
        # + write Hpl, the 64-byte edge record of the pose pass, Hll / bl
        "k_build_edges": 17.0 * E + meas + blk * E + 64.0 * E + 96.0 * L + 56.0 * P + 24.0 * L,  # (+ T, invHll and the
        # landmark lines of the fused iterations: added where the line is assembled, by the share of such iterations)
        "k_build_poses": 64.0 * E + 4.0 * E + 336.0 * P,
        # the pose pass of the fused iteration: records + list entries + one {invHll, z} line per landmark;
        # writes the diagonal block, bp and bsc of every pose
        "k_pose_schur": 64.0 * E + 4.0 * E + 72.0 * L + 384.0 * P,
        # read Hpl, Hll, bl + write T, invHll
        "k_schur_edges": 2 * blk * E + 5.0 * E + 168.0 * L,
        # the H-side of the Schur complement reads T and Hpl of every edge once and writes B blocks;
        # SURVEY 8(d) counts 288 E + 288 B for the whole H-side: split over the two kernels
        "k_hsc_offdiag": blk * E + 288.0 * max(B - P, 0),
        "k_hsc_diag": blk * E + 288.0 * P + 288.0 * P + 48.0 * P + 24.0 * L,
        # the same two kernels on the matrix cores (the default): same arrays, same bytes
        "k_hsc_offdiag_mfma": blk * E + 288.0 * max(B - P, 0),
        "k_hsc_diag_mfma": blk * E + 288.0 * P + 288.0 * P + 48.0 * P + 24.0 * L,
        "k_hsc_landmarks": 2 * blk * E + 8.0 * E,
        "k_hsc_reduce": 288.0 * B + 288.0 * P,
        "k_backsubst_landmarks": blk * E + 5.0 * E + 72.0 * L + 24.0 * L + 24.0 * L + 48.0 * L,
    }


def rocprof_averages(workload):
    """average kernel durations (us) of the committed rocprofv3 --kernel-trace --stats summary of
    this command (profiles/<round>_kernel_stats[_<workload>].csv), keyed by the bare kernel name"""
    name = "%s_kernel_stats%s.csv" % (PROFILE_ROUND, "" if workload == "kitti00" else "_" + workload)
    path = os.path.join(ROOT, "profiles", name)
    out = {}
    if not os.path.exists(path):
        return out, None
    acc = {}
    for r in csv.DictReader(open(path)):
        n = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").split("<")[0]
        a = acc.setdefault(n, [0, 0])
        a[0] += int(r["Calls"])
        a[1] += int(r["TotalDurationNs"])
    for n, (calls, tot) in acc.items():
        out[n] = tot / max(calls, 1) / 1e3
    return out, "profiles/" + name


def pmc_traffic(workload):
    name = "%s_pmc_traffic%s.json" % (PROFILE_ROUND, "" if workload == "kitti00" else "_" + workload)
    path = os.path.join(ROOT, "profiles", name)
    try:
        return json.load(open(path))["kernels"], "profiles/" + name
    except Exception:
        return {}, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="kitti00", choices=sorted(WORKLOADS))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the other regimes (optimize-only, initialize-only, re-flattening, "
                         "structure dirty), the kernel-timing passes with their roofline figures, and the CPU "
                         "baseline with its parity check")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU baseline")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: no dirty / optimize-only / event passes (profiling runs)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed (poses, landmarks, chi2 and lambda per LM "
                         "iteration) as DIR/<name>.npy, float64")
    ap.add_argument("--float32", action="store_true",
                    help="fp32-internal mode (BASELINE config 5): float storage of the Hpl / T block streams")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    extras_on = args.full and not args.no_extras

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("launch with torch.distributed.run --nproc-per-node %d" % args.gpus)

    # bind this rank's GPU (LOCAL_RANK) before any kernel, allocation or communicator exists
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    ndev = torch.cuda.device_count()
    torch.cuda.set_device(local_rank % ndev)
    cugo = importlib.import_module("cuda-bundle-adjustment_amd")
    cugo.set_device(local_rank % ndev)  # the library's own hipSetDevice (it may bind another HIP runtime copy)

    comm = None
    exchange_form = None
    if world > 1:
        # torch.distributed is only the rendezvous (unique id, barriers, the max over ranks); the
        # data-path collectives are RCCL calls inside the library, on the solver's stream
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")  # one node: RCCL's bootstrap over loopback
        import datetime
        dist.init_process_group(backend="gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=600))
        # every rank first checks — without entering a collective — that librccl loads and that it has a
        # device of its own.  If some rank cannot, ALL ranks take the host-staged gloo rehearsal path together
        # (value withheld).  If all can, they enter ncclCommInitRank together, each in a helper thread with a
        # deadline: a rank whose init fails or does not return in time reports 0, the ranks agree over gloo, and on
        # disagreement EVERY rank exits non-zero at once (os._exit: a thread stuck inside RCCL cannot be joined) —
        # no rank is left waiting in a collective for one that gave up.
        import ctypes
        import threading
        can = 1.0
        try:
            ctypes.CDLL("librccl.so.1")
        except OSError:
            try:
                ctypes.CDLL("/opt/rocm/lib/librccl.so.1")
            except OSError:
                can = 0.0
        if ndev < world and os.environ.get("CUGO_BENCH_ASSUME_DEVICES") != "1":
            can = 0.0   # RCCL refuses two ranks of one communicator on the same device (the override: a rehearsal of
                        # the refused init itself — every rank must then exit non-zero, see below)
        if os.environ.get("CUGO_BENCH_FORCE_GLOO") == "1":
            can = 0.0   # rehearsal of the fallback path on a box that could run RCCL
        box = [cugo.comm_unique_id() if (rank == 0 and can > 0.5) else None]
        dist.broadcast_object_list(box, src=0)

        def make_comm():
            if os.environ.get("CUGO_BENCH_FAIL_RANK") == str(rank):   # test hook: this rank fails its init
                raise RuntimeError("CUGO_BENCH_FAIL_RANK: induced failure")
            if os.environ.get("CUGO_BENCH_HANG_RANK") == str(rank):   # test hook: this rank never returns
                threading.Event().wait()
            cugo.set_device(local_rank % ndev)   # (the current device is per thread)
            return cugo.Comm(box[0], rank, world)
        how, comm = cugo.create_comm_agreed(dist, rank, world, make_comm, can_try=can > 0.5,
                                            deadline_s=float(os.environ.get("CUGO_BENCH_COMM_TIMEOUT", "180")),
                                            log=lambda m: sys.stderr.write(m + "\n"))
        if how == "failed":
            sys.stderr.write("rank %d: not every rank has a communicator: all ranks exit\n" % rank)
            sys.stderr.flush()
            os._exit(3)
        if how == "fallback":
            exchange_form = ("FALLBACK: callback + torch.distributed gloo through host memory (librccl or one GPU per "
                             "rank not available on every rank): a rehearsal of the sharded path, not a scaling point")
        else:
            exchange_form = ("native: RCCL on the solver's stream inside libcugo_hip.so (ncclAllReduce; with rank-owned "
                             "elimination subtrees ncclReduceScatter + grouped ncclBroadcast)")
    views = {}

    def host_exchange(ptr, n, op):
        class _DevPtr:
            def __init__(self, p, k):
                self.__cuda_array_interface__ = {"data": (int(p), False), "shape": (int(k),), "typestr": "<f8",
                                                 "version": 2}
        t = views.get((ptr, n))
        if t is None:
            t = views[(ptr, n)] = torch.as_tensor(_DevPtr(ptr, n), device="cuda")
        h = t.cpu()
        if op >= 2:   # broadcast from rank op - 2 (rank-owned elimination subtrees)
            dist.broadcast(h, src=op - 2)
        elif op == -1:  # reduce-scatter of `world` equal segments (ownership-keyed exchange of the Schur system)
            seg = n // world
            # gloo has no reduce-scatter: all-reduce on the host, keep the own segment (a rehearsal path only)
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            own = h[rank * seg:(rank + 1) * seg].clone()
            h.fill_(float("nan"))
            h[rank * seg:(rank + 1) * seg] = own
        else:
            dist.all_reduce(h, op=dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MAX)
        t.copy_(h)
        torch.cuda.synchronize()

    P, L, E, seed, nlc, stereo = WORKLOADS[args.workload]
    data = cugo.synth(P, L, E, seed=seed, n_loop_closures=nlc, stereo_fraction=stereo)
    pose_ids = np.arange(P, dtype=np.int32)
    lm_ids = np.arange(L, dtype=np.int32)

    def new_graph():
        g = cugo.graph_from_arrays(data)
        if args.float32:
            g.set_float32(True)
        if comm is not None:
            g.set_comm(comm)
        elif world > 1:
            g.set_shard(rank, world, host_exchange)
        return g

    def reset(g):
        g.set_poses(pose_ids, data["pose"])
        g.set_landmarks(lm_ids, data["lm"])

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if world > 1:
            t = torch.tensor([x], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        return x

    # ---- a pool of optimisers, each warmed up the way the reference sample does it ------------
    # One optimiser per step up to POOL_MAX steps; beyond that the steps cycle over the pool, so that the set-up
    # (graph, flattening, structure, ordering, symbolic factor per optimiser) and the memory do not grow with --steps.
    graphs, cold = [], None
    for gi in range(min(args.steps, POOL_MAX)):
        g = new_graph()
        t0 = time.perf_counter()
        g.initialize()
        t1 = time.perf_counter()
        g.optimize(1)
        t2 = time.perf_counter()
        if gi == 0:  # first-ever call: allocations, module load, structure build, ordering, symbolic
            cold = {"initialize_ms": (t1 - t0) * 1e3, "optimize1_ms": (t2 - t1) * 1e3,
                    "host_phase_ms": {k: v for k, v in g.time_profile().items() if v > 0}}
        reset(g)
        graphs.append(g)
    for i in range(args.warmup):
        g = graphs[i % len(graphs)]
        g.initialize()
        g.optimize(args.iters)
        reset(g)
    timed = graphs

    # ---- headline: K initialize()+optimize(10), structure clean, contiguous within each pass over the pool ----
    # (every optimiser starts a step from the reset estimates; between two passes the pool is reset, untimed)
    elapsed, iters_total, left, last = 0.0, 0, args.steps, None
    while left > 0:
        run = timed[:min(left, len(timed))]
        if last is not None:
            for g in run:
                reset(g)
        barrier()
        t0 = time.perf_counter()
        for g in run:
            g.initialize()
            g.optimize(args.iters)
        barrier()
        elapsed += max_over_ranks(time.perf_counter() - t0)
        iters_total += sum(len(g.stats()) for g in run)
        left -= len(run)
        last = run[-1]

    stats = [g.stats() for g in timed]
    nedges = timed[0].n_active_edges()
    sstats = timed[0].structure_stats()
    gpu_chi = [s["chi2"] for s in stats[0]]
    gpu_pose, gpu_lm = timed[0].poses(), timed[0].landmarks()
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from the last step: estimates by id and the LM trace
        os.makedirs(args.dump_outputs, exist_ok=True)
        trace = last.stats()
        outputs = {"poses": last.poses(), "landmarks": last.landmarks(),
                   "chi2": [s["chi2"] for s in trace], "lambda": [s["lam"] for s in trace]}
        for name, a in outputs.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), np.asarray(a, dtype=np.float64))
    xstats = timed[0].exchange_stats() if world > 1 else None
    # every rank must have taken the same LM decisions and ended every iteration on the same chi2 (the exchanged
    # sums are the same bits on every rank): checked over the rendezvous group, reported in the line
    ranks_agree = None
    if world > 1:
        mine = torch.tensor([s["chi2"] for st in stats for s in st] + [float(s["trials"]) for st in stats for s in st],
                            dtype=torch.float64)
        n_mine = torch.tensor([mine.numel()], dtype=torch.int64)
        n_all = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(n_all, n_mine)
        ranks_agree = all(int(t.item()) == mine.numel() for t in n_all)
        if ranks_agree:
            every = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(every, mine)
            ranks_agree = all(torch.equal(t, every[0]) for t in every)

    extras = {}
    if extras_on:
        # ---- optimize(10) alone, inputs resident in HBM --------------------------------------
        for g in timed:
            reset(g)
            g.initialize()
        barrier()
        t0 = time.perf_counter()
        for g in timed:
            g.optimize(args.iters)
        barrier()
        el_opt = max_over_ranks(time.perf_counter() - t0)
        it_opt = sum(len(g.stats()) for g in timed)
        # ---- initialize() alone ---------------------------------------------------------------
        for g in timed:
            reset(g)
        barrier()
        t0 = time.perf_counter()
        for g in timed:
            g.initialize()
        barrier()
        el_init = max_over_ranks(time.perf_counter() - t0)
        # ---- full re-flattening (as after any change to an edge or a fixed flag), structure kept -
        for g in timed:
            g.set_option("flatten_reuse", 0)
            reset(g)
        barrier()
        t0 = time.perf_counter()
        for g in timed:
            g.initialize()
            g.optimize(args.iters)
        barrier()
        el_flat = max_over_ranks(time.perf_counter() - t0)
        it_flat = sum(len(g.stats()) for g in timed)
        for g in timed:
            g.set_option("flatten_reuse", 1)
            reset(g)
        # ---- structure dirty: pattern + ordering + symbolic analysis inside the step ---------
        nd = min(len(timed), 3)
        for g in timed[:nd]:
            g.set_option("structure_reuse", 0)
        barrier()
        t0 = time.perf_counter()
        for g in timed[:nd]:
            g.initialize()
            g.optimize(args.iters)
        barrier()
        el_dirty = max_over_ranks(time.perf_counter() - t0)
        it_dirty = sum(len(g.stats()) for g in timed[:nd])
        dirty_profile = timed[0].time_profile()
        for g in timed[:nd]:
            g.set_option("structure_reuse", 1)
        extras = {
            "optimize_only": {"ms_per_step": el_opt / len(timed) * 1e3, "value": nedges * it_opt / el_opt,
                              "note": "optimize(%d) alone, flattened graph resident in HBM" % args.iters},
            "initialize_only_ms": el_init / len(timed) * 1e3,
            "reflatten": {"ms_per_step": el_flat / len(timed) * 1e3, "value": nedges * it_flat / el_flat,
                          "note": "initialize()+optimize(%d) with CUGO_NO_FLATTEN_REUSE=1: the whole pointer graph is "
                                  "flattened and uploaded again in every step (what a changed edge or fixed flag "
                                  "costs); the headline's initialize() finds the graph unchanged since the warm-up "
                                  "(change counters of the vertex / edge sets) and uploads only the estimates"
                                  % args.iters},
            "structure_dirty": {"ms_per_step": el_dirty / nd * 1e3, "value": nedges * it_dirty / el_dirty,
                                "steps": nd,
                                "host_phase_ms_sum_over_steps": {k: v for k, v in dirty_profile.items() if v > 0},
                                "note": "initialize()+optimize(%d) with CUGO_NO_STRUCTURE_REUSE=1: Hsc pattern, "
                                        "product lists, ordering and symbolic factor rebuilt in every step; host_phase_ms: the host-side "
                                        "phases (the device phases are only timed under CUGO_PROFILE=1)" % args.iters},
        }
    for g in graphs:
        g.close()

    # ---- device time by kernel group and by kernel: HIP events on the solver's stream, two passes of their own ---
    # pass A (groups): ONE event per group boundary, so the group times add up exactly to the device time of that
    # optimize(10) — figures that fit inside the step; pass B (kernels): an event pair round every launch.  A pair
    # brackets the kernel AND its dispatch (1 - 2 us that an un-instrumented stream hides behind the kernel before):
    # the per-kernel averages are upper bounds of the kernel durations, fractions computed from them lower bounds;
    # the rocprofv3 average of the same kernel (committed trace) and the fraction it gives are printed beside them
    groups, kernels, roofline = {}, {}, None
    groups_fit = None
    if extras_on:
        gk = new_graph()
        gk.initialize()
        gk.optimize(1)
        reset(gk)
        gk.initialize()
        gk.set_kernel_timing(2)
        tA = time.perf_counter()
        gk.optimize(args.iters)
        passA_ms = (time.perf_counter() - tA) * 1e3
        gtimes = gk.kernel_times()
        reset(gk)
        gk.initialize()
        gk.set_kernel_timing(1)
        gk.optimize(args.iters)
        ktimes = {k: v for k, v in gk.kernel_times().items() if k.startswith("k_")}
        gk.close()
        ktimes.update({k: v for k, v in gtimes.items() if not k.startswith("k_")})
        shard = max(1, world)
        n_fact = max(1, ktimes.get("cholesky", {}).get("launches", 1))
        El, Ll, Pf, B = nedges / shard, L / shard, P - 1, sstats["hsc_blocks"]
        Es = float(np.count_nonzero(data["e_stereo"])) / shard
        comp = compulsory_bytes(El, El - Es, Es, Pf, Ll, B, args.float32)
        if os.environ.get("CUGO_FUSE_T", "1") != "0" and not os.environ.get("CUGO_SCHUR_PLAN"):
            # from the second LM iteration on the build pass also writes T and invHll
            # two-stream form (CUGO_POSE_SCHUR=0): + T and invHll; one-stream form (the default): G in place of Hpl — no
            # block bytes on top — and the 72-byte line {L^-1, y} per landmark in place of invHll
            if os.environ.get("CUGO_POSE_SCHUR", "1") != "0":
                comp["k_build_edges"] += 72.0 * Ll * (args.iters - 1) / args.iters
            else:
                comp["k_build_edges"] += ((72.0 if args.float32 else 144.0) * El + 72.0 * Ll) * (args.iters - 1) / args.iters
        flops = {"k_up_potrf": sstats.get("up_potrf_flops", 0.0)}
        # the trsm / syrk work of a factorisation is spread over four kernels (fused 64x64 and 32x32 tiles,
        # and the two-phase pair of the wide levels): rated together, against the non-redundant flop count
        tile_kernels = ("k_up_trsyrk", "k_up_trsyrk32", "k_up_trsm", "k_up_syrk")
        tile_flops = sstats.get("up_trsm_flops", 0.0) + sstats.get("up_syrk_flops", 0.0)
        rp_avg, rp_src = rocprof_averages(args.workload)
        pmc, pmc_src = pmc_traffic(args.workload)
        for name, kt in ktimes.items():
            if kt["launches"] == 0:
                continue
            avg_ms = kt["ms"] / kt["launches"]
            ent = {"avg_ms": avg_ms, "launches": kt["launches"], "total_ms": kt["ms"]}
            if name.startswith("k_"):

                if name in rp_avg:
                    ent["rocprof_avg_us"] = rp_avg[name]
                if name in pmc and world == 1 and not args.float32:
                    ent["traffic"] = pmc[name]["hbm_bytes_per_launch_fetch_x2"]
                if name in comp:
                    ent.update(bound="hbm", alg_bytes=comp[name], achieved=comp[name] / (avg_ms * 1e-3) / 1e9,
                               peak=HBM_PEAK_GBS, unit="GB/s")
                elif name in flops:
                    # flops of ONE factorisation over the launches of one factorisation
                    per_launch = flops[name] * n_fact / kt["launches"]
                    ent.update(bound="mfma", alg_flops=per_launch, achieved=per_launch / (avg_ms * 1e-3) / 1e12,
                               peak=FP64_PEAK_TFLOPS, unit="TFLOP/s")
                if "achieved" in ent:
                    ent["frac"] = ent["achieved"] / ent["peak"]
                    if "rocprof_avg_us" in ent:  # the same count over the committed rocprofv3 average
                        ent["frac_from_rocprof_avg"] = ent["frac"] * avg_ms / (ent["rocprof_avg_us"] * 1e-3)
                kernels[name] = ent
                continue
            sb = survey_bytes(name, El, Pf, Ll, B)
            if sb is not None:
                ent.update(bound="hbm", alg_bytes_survey_8d=sb, achieved=sb / (avg_ms * 1e-3) / 1e9,
                           peak=HBM_PEAK_GBS, unit="GB/s")
            elif name == "cholesky":
                ent.update(bound="mfma", alg_flops=sstats["chol_flops"],
                           achieved=sstats["chol_flops"] / (avg_ms * 1e-3) / 1e12, peak=FP64_PEAK_TFLOPS, unit="TFLOP/s")
            elif name == "exchange" and xstats:
                ent.update(bytes_per_call=xstats["bytes"] / max(xstats["calls"], 1))
            if "achieved" in ent:
                ent["frac"] = ent["achieved"] / ent["peak"]
                if ent["frac"] > 1.0:  # a fused pass moves fewer bytes than SURVEY 8(d) counts for it
                    ent["note"] = "moves fewer bytes than the SURVEY 8(d) count; see the kernel entries"
                    ent["frac"] = None
            groups[name] = ent
        tk = [kernels[k] for k in tile_kernels if k in kernels]
        if tk and tile_flops > 0:
            tot_ms = sum(k["total_ms"] for k in tk)
            kernels["k_up_tiles (sum of %s)" % ", ".join(k for k in tile_kernels if k in kernels)] = {
                "total_ms": tot_ms, "launches": sum(k["launches"] for k in tk), "bound": "mfma",
                "alg_flops_per_factorisation": tile_flops,
                "achieved": tile_flops * n_fact / (tot_ms * 1e-3) / 1e12, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": tile_flops * n_fact / (tot_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                "avg_ms": tot_ms / max(1, sum(k["launches"] for k in tk))}
        # the groups come from pass A: they add up to the device time of its optimize(10), which fits in the step
        gsum = sum(v["total_ms"] for v in groups.values())
        groups_fit = {"sum_of_groups_ms": gsum, "pass_wall_ms": passA_ms, "ms_per_step": elapsed / args.steps * 1e3,
                      "fits": bool(gsum <= passA_ms * 1.001 and gsum <= elapsed / args.steps * 1e3 * 1.02),
                      "note": "groups: one event per group boundary in a pass of its own (their sum is the device time "
                              "between the first and the last event of optimize()); kernels: event pairs per launch in "
                              "another pass (upper bounds of the kernel durations: a pair brackets the dispatch as well)"}
        rated = {k: v for k, v in kernels.items() if "achieved" in v}
        if rated:
            dominant = max(rated, key=lambda k: rated[k]["total_ms"])
            d = rated[dominant]
            roofline = {"kernel": dominant, "bound": d["bound"], "achieved": d["achieved"], "peak": d["peak"],
                        "unit": d["unit"], "frac": d["frac"], "traffic": d.get("traffic"),
                        "traffic_source": (pmc_src + " (FETCH_SIZE x2 + WRITE_SIZE, separate --pmc passes)")
                        if d.get("traffic") else None,
                        "avg_launch_ms": d["avg_ms"], "launches": d["launches"],
                        "rocprof_avg_us": d.get("rocprof_avg_us"), "rocprof_source": rp_src,
                        "frac_from_rocprof_avg": d.get("frac_from_rocprof_avg"),
                        "timing": "HIP event pairs on the solver's stream in a separate pass of optimize(%d): a pair "
                                  "brackets the kernel and its dispatch (1 - 2 us that an un-instrumented stream hides), so "
                                  "avg_launch_ms is an upper bound and frac a lower bound; rocprof_avg_us is the same "
                                  "kernel in the committed rocprofv3 trace" % args.iters,
                        "note": "fp64 MFMA peak == fp64 vector peak (78.6 TF) on MI355X; the multifrontal "
                                "Cholesky kernels are latency / critical-path bound (DESIGN.md section 5)"}

    # ---- CPU baseline: the oracle (restatement of the g2o-style path), same graph, same region ----
    cpu = None
    parity = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        import oracle

        def problem():
            return oracle.Problem(data["pose"], data["pose_fixed"], data["lm"], data["lm_fixed"], data["e_pose"],
                                  data["e_lm"], data["e_stereo"], data["e_meas"], data["e_omega"], data["e_cam"])
        cpu_iters = args.iters if E <= 1000000 else 2
        prob = problem()
        tc = time.perf_counter()
        ref = prob.optimize(cpu_iters)   # the parity checker: -O2 -ffp-contract=off, 1 thread, fixed order
        checker_s = time.perf_counter() - tc
        nref = min(len(ref), len(gpu_chi))
        rel = max(abs(gpu_chi[i] - ref[i]["chi2"]) / abs(ref[i]["chi2"]) for i in range(nref))
        parity = {"max_rel_chi2_diff_vs_cpu": rel, "iterations_compared": nref}
        if cpu_iters == args.iters:
            parity.update(rmse_rotation=float(np.sqrt(np.mean((gpu_pose[:, :4] - prob.pose[:, :4]) ** 2))),
                          rmse_translation=float(np.sqrt(np.mean((gpu_pose[:, 4:] - prob.pose[:, 4:]) ** 2))),
                          rmse_landmark=float(np.sqrt(np.mean((gpu_lm - prob.lm) ** 2))))
        # timed legs: the same source built -O3 -march=native on this host (no OpenMP for the
        # 1-thread leg: its atomics cost even when alone), then with OpenMP over edges / landmarks at
        # 8, 16, ... up to all host cores: the best is reported, every leg is listed
        ncores = os.cpu_count() or 1
        try:
            ncores = len(os.sched_getaffinity(0))
        except Exception:
            pass
        legs = {}

        def leg(label, lib, nt):
            pr = problem()
            tc = time.perf_counter()
            r = pr.optimize(cpu_iters, use_lib=lib)
            s = time.perf_counter() - tc
            legs[label] = {"seconds": s, "threads": nt, "value": nedges * len(r) / s}
        leg("1_thread", oracle.fast_lib(openmp=False), 1)
        import ctypes
        fast = oracle.fast_lib(openmp=True)
        omp = ctypes.CDLL("libgomp.so.1")
        for nt in sorted(set([min(8, ncores), min(16, ncores), min(32, ncores), ncores])):
            omp.omp_set_num_threads(nt)
            leg("openmp_%d_threads" % nt, fast, nt)
        cpu_model = ""
        try:
            cpu_model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
        except Exception:
            pass
        best = max(legs.values(), key=lambda v: v["value"])
        cpu = {"value": best["value"], "unit": "edge*iter/s", "cores": best["threads"], "kind": "port",
               "seconds": best["seconds"], "legs": legs, "nproc": ncores, "cpu_model": cpu_model,
               "checker_seconds_O2_1thread": checker_s,
               "build": "gcc -O3 -march=native [-fopenmp -DBA_OMP] oracle/ba_oracle.c (compiled on this host)",
               "sample": "%s-shaped graph, %d LM iterations incl. structure build + ordering + symbolic "
                         "(a cold call: the CPU restatement keeps nothing between calls), oracle/ba_oracle.c; "
                         "OpenMP over edges / landmarks, the sparse LL^T and the ordering are sequential"
                         % (args.workload, len(ref))}

    if rank == 0:
        chol_share = None
        if "cholesky" in groups and extras_on:
            # from the boundary-event pass: the groups add up to the device time of optimize()
            tot = sum(v["total_ms"] for k, v in groups.items() if k != "exchange")
            chol_share = groups["cholesky"]["total_ms"] / max(tot, 1e-9)
        out = {
            "metric": "ba_edge_iterations_per_sec", "value": nedges * iters_total / elapsed,
            "unit": "edge*iter/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "%s-shaped synthetic graph: %d poses / %d landmarks / %d edges, %d LM iterations"
                                   % (args.workload, P, L, nedges, args.iters),
                       "timed_region": "initialize(); optimize(%d) per step, contiguous (ref "
                                       "samples/sample_ba_from_file/main.cpp:185-190), structure clean" % args.iters,
                       "parallelism": ("landmark-sharded x%d; per LM trial the Schur system [Hsc|bsc] is exchanged by RCCL on "
                                       "the solver's stream — all-reduce with the LL^T replicated, or (graphs with >= "
                                       "CUGO_OWN_MIN_GFLOP per factorisation) reduce-scatter keyed on front ownership "
                                       "with the LL^T split into rank-owned elimination subtrees under a replicated top"
                                       % world) if world > 1 else "single GPU",
                       "lm_iterations_per_step": iters_total / args.steps,
                       "block_storage": "float (Hpl, Hpl*invHll streams; BASELINE config 5)" if args.float32 else "double"},
            "ba_10iter_seconds": elapsed / args.steps,
            "cold_first_call": cold,
            "roofline": roofline,
            "cpu_baseline": cpu,
            "parity": parity,
            "kernel_groups": groups,
            "kernel_groups_fit_the_step": groups_fit,
            "kernels": kernels,
            "structure": sstats,
            "chi2": gpu_chi,
        }
        out.update(extras)
        # the regimes a caller can be in, beside the headline (config survives the driver's parsing):
        # ORB-SLAM2 builds a new graph per BA call, i.e. pays `structure_dirty`
        # (scalar keys: a nested dict does not survive the driver's parsing of `config`)
        out["config"]["regime_headline_ms"] = elapsed / args.steps * 1e3
        out["config"]["regime_reflatten_ms"] = extras.get("reflatten", {}).get("ms_per_step")
        out["config"]["regime_new_graph_ms"] = extras.get("structure_dirty", {}).get("ms_per_step")
        out["config"]["regime_optimize_only_ms"] = extras.get("optimize_only", {}).get("ms_per_step")
        out["config"]["regime_cold_first_call_ms"] = (cold["initialize_ms"] + cold["optimize1_ms"]) if cold else None
        if world > 1 and comm is None:
            # a run that fell back to host staging through gloo is not a scaling point: no throughput
            out["value"] = None
            out["invalid"] = "native RCCL communicator unavailable: host-staged gloo fallback, value withheld"
        if world > 1 and xstats:
            trials = sum(max(s["trials"], 0) + 1 for s in stats[0])
            out["ranks_agree_bitwise_on_chi2_and_trials"] = ranks_agree
            if not ranks_agree:
                out["value"] = None
                out["invalid"] = "the ranks ended on different chi2 / trial counts"
            out["exchange"] = {"form": exchange_form, "calls_per_step": xstats["calls"], "bytes_per_step": xstats["bytes"],
                               "payload_bytes_per_trial": 8.0 * (36 * sstats["hsc_blocks"] + 6 * (P - 1)) + 16.0,
                               "schur_system_bytes_received_per_rank_and_trial": sstats.get("xchg_sys_bytes"),
                               "schur_system_bytes_full_allreduce": sstats.get("xchg_sys_full_bytes"),
                               "schur_system_exchange": ("reduce-scatter keyed on front ownership + all-reduce of the top's part"
                                                         if sstats.get("xchg_sys_bytes", 0) < sstats.get("xchg_sys_full_bytes", 0)
                                                         else "all-reduce (replicated factorisation)"),
                               "trials_per_step": trials,
                               "cholesky": {"rank_flops": sstats.get("chol_rank_flops"),
                                            "replicated_top_flops": sstats.get("chol_top_flops"),
                                            "broadcast_bytes_per_trial": sstats.get("chol_bcast_bytes"),
                                            "broadcasts_per_trial": sstats.get("chol_bcasts"),
                                            "cholesky_share_of_step": chol_share,
                                            "note": "the sparse LL^T runs by rank-owned elimination subtrees: a rank "
                                                    "factors its own subtrees (rank_flops, rank 0's here) and the "
                                                    "replicated top of the tree; only the top's share of the "
                                                    "factorisation stays serial in the Amdahl sense, and on graphs "
                                                    "whose levels are latency-bound (kitti_00) the per-level critical "
                                                    "path does not shrink with fewer fronts per level"}}
        elif chol_share is not None:
            out["amdahl"] = {"replicated_cholesky_share_of_optimize": chol_share,
                             "max_speedup_8_gpus": 1.0 / (chol_share + (1 - chol_share) / 8)}
        print(json.dumps(out))
    if comm is not None:
        barrier()
        comm.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
