#!/usr/bin/env python3
"""Headline benchmark: depth-pair alignments/second (640x480, 10 Gauss-Newton iterations) on N MI355X.

Workload (BASELINE.json configs[3] sharded as SURVEY.md §8(e) prescribes; at N=8 it is exactly the
1024-pair loop-closure batch, at N=1 it is one GPU's 128-pair shard): every rank owns `--pairs`
independent synthetic VGA depth pairs, resident in HBM as uint16 millimetre frames when the timed region
starts.  One step = for every pair: DepthImage_convert_16UC1_to_32FC1 + DepthImageConverterIntegralImage::compute
on both frames, then Aligner::align (10 outer x 1 inner iterations), then an all-gather of the result records
(RCCL when N > 1).  Nothing is cached between steps.

`python bench.py --gpus N` without a torchrun environment starts the N ranks itself (one process per GPU, before
anything touches a GPU); under `python -m torch.distributed.run ... bench.py --gpus N` it is one of the N ranks.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the steps, writes `--dump-outputs` if asked and
prints the contract fields and `config`: nothing else.  With `--full` the line also carries `roofline` (dominant kernel,
hipEvent timing of a serial profiled pass), `gather` (the assembled records checked against the rank's own and against
the committed single-GPU digests), `multi_gpu` (N > 1), `cpu_baseline` (the CPU oracle = a port of the reference path,
timed on this box's host cores on a bounded sample of the same workload) and, at N = 1, the other lines of SURVEY.md
§8(d) as extra keys: `chi2_match`, `align_only`, `closure_match_batch` (the loop-closure call proper: non-identity
guesses + matchClouds scores), `config5_1280x960`, `tracker_config2` (BASELINE configs[2]: 200-frame VGA stream through
PwnTracker::processFrame).  The --no-* options leave out parts of a --full run.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FREE_RUNNING_CHI2_BAR = 5e-4   # free-running chi2 trace vs the fp64-accumulating oracle at VGA (tests/test_gpu_parity.py: FREE_CHI2_RTOL_VGA: measured worst 1.9e-4
                               # over 16 seeds, each excess with 1-3 flipped correspondences); the 1e-5 of north_star holds teacher-forced (measured 6e-8)
HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6 TB/s is what a bare streaming read gets on these boxes


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=128, help="depth pairs per GPU (weak scaling)")
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--sub-frames", type=int, default=int(os.environ.get("PWN_SUB_FRAMES", 64)))
    ap.add_argument("--sub-pairs", type=int, default=int(os.environ.get("PWN_SUB_PAIRS", 64)))
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: CPU baseline, serial profiled pass (roofline), record checks, multi-GPU diagnostics, "
                         "latency, chi2 gate, bandwidth probe and the extra lines; off: the timed steps and the result line only")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget of each leg of the CPU baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the extra bench lines (align_only, closure_match_batch, config5, tracker)")
    ap.add_argument("--no-config5", action="store_true")
    ap.add_argument("--no-tracker", action="store_true")
    ap.add_argument("--tracker-frames", type=int, default=200)
    ap.add_argument("--cpu-baseline-only", action="store_true", help="(internal) run only the CPU baseline leg and print its JSON")
    ap.add_argument("--no-profile", action="store_true", help="skip the serial profiled pass (roofline fields become 0)")
    ap.add_argument("--omega-storage", choices=("exact9", "sym6"), default=os.environ.get("PWN_OMEGA_STORAGE", "sym6"),
                    help="storage of the clouds' point information matrices in the batch workload (include/pwn_hip.h: pwn_hip_ctx_set_omega_storage)")
    ap.add_argument("--step-mode", choices=("fused", "split"), default=os.environ.get("PWN_STEP_MODE", "fused"),
                    help="fused: one submission per step (pwn_hip_convert_align_batch_u16: sub-batch k converts while k-1 aligns); split: convert_batch_u16, then "
                         "align_batch_records (a host wait between the halves).  Same results bit for bit; the records are packed on the device in both")
    ap.add_argument("--streams", type=int, default=4, help="HIP streams the batch calls use in the timed region (1 = serial)")
    ap.add_argument("--render-workers", type=int, default=0,
                    help="processes that render the synthetic frames (0 = automatic; 1 = in this process: required under rocprofv3, whose preloaded "
                         "library has initialised the GPU before Python starts -- no child process may be started from such a process)")
    ap.add_argument("--total-pairs", type=int, default=0,
                    help="strong-scaling mode: shard the SAME list of this many pairs (BASELINE configs[3]: 1024) over the N ranks, instead of --pairs per rank")
    ap.add_argument("--write-records-crc", action="store_true",
                    help="N = 1 only: write profiles/records_crc.json (per-pair CRC32 of the result records) -- multi-GPU runs check their assembled records against it")
    ap.add_argument("--check-gather", action="store_true", help="kept for scripts: the `gather` object (backend, records, equality with the local records) is in every --full line")
    ap.add_argument("--partition-serial", action="store_true",
                    help="--mode partition without the look-ahead: convert `current`, export, broadcast the buffer's bound, import, match -- one after the other "
                         "(round 5's step; the default converts and broadcasts the next keyframes beside the matches)")
    ap.add_argument("--mode", choices=("pairs", "partition"), default="pairs",
                    help="pairs (default, the headline): independent fresh pairs, convert 2 frames + align each.  partition: PwnCloser::processPartition "
                         "(pwn_tracker/pwn_closer.cpp:85-111; SURVEY.md 8(e)) -- ONE `current` frame against the cached clouds of the other partition: every rank "
                         "converts and caches its shard of --pairs keyframes per GPU once (untimed); a step = rank 0 converts `current`, its cloud is replicated "
                         "to every GPU by one broadcast (RCCL), every rank runs matchClouds (align from an odometry guess + depth-agreement score) of `current` "
                         "against its shard, 288-byte records all-gathered")
    ap.add_argument("--gather-after-call", action="store_true",
                    help="pairs mode, N > 1: queue the records' all-gather after the step's library call has returned (rounds 1-5) instead of from inside it "
                         "(pwn_hip_ctx_set_enqueued_callback); for the A/B")
    ap.add_argument("--one-device", action="store_true",
                    help="rehearsal of N > 1 on ONE GPU: every rank is a process of its own on device 0 and the collectives go through gloo (RCCL refuses two "
                         "ranks on one device).  Same steps, same ordering calls (pwn_hip_ctx_wait_stream / _signal_stream), the ranks contend for the device; "
                         "the rate is not a scaling figure and the line says so (config.rehearsal)")
    ap.add_argument("--dry-run-cpu", action="store_true",
                    help="launcher / sharding / gather plumbing only, on the CPU with the gloo backend (no GPU, no kernels): used by tests")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="rank 0: write what the last timed step returned (the result fields of the rank's pairs and the assembled records of every "
                         "pair) as DIR/<name>.npy, float32 / float64, at most 64 MB in all -- for comparing two builds output for output")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def conf(rows, cols):
    from g2o_frontend_amd import synth
    from g2o_frontend_amd import conf as C      # the reference's configuration files as tables (the oracle is not imported by the GPU-driving process)
    if (rows, cols) == (960, 1280):
        K = synth.K_1280
        conv = dict(C.K2_CONF_CONVERTER)
    else:
        K = synth.K_VGA if (rows, cols) == (480, 640) else synth.scaled_K(synth.K_VGA, 640 // cols)
        conv = dict(C.VGA_CONF_CONVERTER)
    return K, conv, dict(C.VGA_CONF_ALIGNER)


def build_objects(ctx, rows, cols, K, conv, alig):
    from g2o_frontend_amd import api
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    proj.setMinDistance(conv["min_distance"]); proj.setMaxDistance(conv["max_distance"]); proj.setImageSize(rows, cols)
    st = api.StatsCalculatorIntegralImage()
    st.setWorldRadius(conv["world_radius"]); st.setMinImageRadius(conv["min_image_radius"]); st.setMaxImageRadius(conv["max_image_radius"])
    st.setMinPoints(conv["min_points"]); st.setCurvatureThreshold(conv["stats_curvature_threshold"])
    pi, ni = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
    pi.setCurvatureThreshold(conv["point_info_curvature_threshold"]); ni.setCurvatureThreshold(conv["normal_info_curvature_threshold"])
    converter = api.DepthImageConverterIntegralImage(proj, st, pi, ni)
    f = api.CorrespondenceFinder()
    f.setInlierDistanceThreshold(alig["inlier_distance_threshold"]); f.setInlierNormalAngularThreshold(alig["inlier_normal_angular_threshold"])
    f.setFlatCurvatureThreshold(alig["flat_curvature_threshold"]); f.setInlierCurvatureRatioThreshold(alig["inlier_curvature_ratio_threshold"])
    f.setImageSize(rows, cols)
    lin = api.Linearizer(); lin.setInlierMaxChi2(alig["inlier_max_chi2"]); lin.setRobustKernel(alig["robust_kernel"])
    al = api.Aligner(ctx)
    al.setProjector(proj); al.setLinearizer(lin); al.setCorrespondenceFinder(f)
    al.setOuterIterations(alig["outer_iterations"]); al.setInnerIterations(alig["inner_iterations"])
    return converter, al


# ------------------------------------------------------------------------------------------------ launcher (N > 1 without torchrun)
def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def cpu_topology():
    """{package id: sorted cpus} of the cpus this process may run on (sysfs; one package when sysfs does not say)"""
    pk = {}
    for c in sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else range(os.cpu_count() or 1):
        try:
            with open(f"/sys/devices/system/cpu/cpu{c}/topology/physical_package_id") as f:
                k = int(f.read().strip())
        except Exception:
            k = 0
        pk.setdefault(k, []).append(c)
    return pk


def rank_cpus(local_rank: int, n_local: int, topo=None):
    """The cpus of one rank: the ranks of a node get DISJOINT, contiguous blocks, the first half of the ranks on the first socket and so on (GPUs
    0..n/2-1 hang off socket 0 on the 8-GPU nodes), so that a rank's render pool and runtime threads neither migrate across sockets nor fight the
    other ranks' for cores.  [] = leave the affinity alone (fewer cpus than ranks)."""
    topo = cpu_topology() if topo is None else topo
    packs = [sorted(topo[k]) for k in sorted(topo)]
    if n_local <= 1 or sum(len(p) for p in packs) < n_local:
        return []
    if len(packs) > 1 and n_local % len(packs) == 0 and all(len(p) >= n_local // len(packs) for p in packs):
        per = n_local // len(packs)
        cpus, r, m = packs[local_rank // per], local_rank % per, per
    else:
        cpus, r, m = [c for p in packs for c in p], local_rank, n_local
    lo, hi = (r * len(cpus)) // m, ((r + 1) * len(cpus)) // m
    return cpus[lo:hi]


def pin_rank(local_rank: int, n_local: int):
    """called first thing in a rank, before anything touches the GPU (no wrapper process, no exec)"""
    if os.environ.get("PWN_BENCH_NO_AFFINITY") == "1" or not hasattr(os, "sched_setaffinity"):
        return None
    cpus = rank_cpus(local_rank, n_local)
    if cpus:
        try:
            os.sched_setaffinity(0, cpus)
        except OSError:
            return None
    return cpus


def launch_ranks(n: int, argv) -> int:
    """One child process per GPU, started before this process has touched a GPU (it never does).  Rank 0's stdout is this
    process's stdout (the one JSON line); the other ranks' stdout goes to stderr.  Returns the worst exit code."""
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=None if r == 0 else sys.stderr))
    rc = 0
    alive = list(procs)
    while alive:
        time.sleep(0.2)
        for p in list(alive):
            code = p.poll()
            if code is None:
                continue
            alive.remove(p)
            if code != 0 and rc == 0:
                rc = code
                for q in alive:          # a rank failed: the others would wait in a collective for ever
                    q.terminate()
    return rc


# ------------------------------------------------------------------------------------------------ input rendering (CPU, before GPU init)
def _render_job(job):
    from g2o_frontend_amd import synth
    kind = job[0]
    if kind == "pair":
        _, seed, rows, cols, K = job
        ref_mm, cur_mm, _ = synth.make_pair(seed, rows, cols, K)
        return ref_mm, cur_mm
    _, seed, pose, rows, cols, K, hole_stream = job
    return synth.render_depth_mm(seed, np.asarray(pose), rows, cols, K, hole_stream=hole_stream)


def render_all(jobs, world, workers=0):
    """the synthetic uint16 frames of all jobs, rendered by a pool of CPU processes (spawned before the GPU is initialised)"""
    import concurrent.futures as cf
    import multiprocessing as mp
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    workers = max(1, min(16, ncpu // max(world, 1), len(jobs))) if workers <= 0 else workers
    if workers == 1:
        return [_render_job(j) for j in jobs]
    with cf.ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(_render_job, jobs, chunksize=max(1, len(jobs) // (4 * workers))))


# ------------------------------------------------------------------------------------------------ CPU baseline (child process)
def _cpu_pairs_loop(O, synth, rows, cols, K, cp, apar, seeds, budget_s):
    done, t_conv, t_align, t0 = 0, 0.0, 0.0, time.perf_counter()
    for s in seeds:
        ref_mm, cur_mm, _ = synth.make_pair(s, rows, cols, K)          # rendering is not part of the measured work
        a = time.perf_counter()
        cr, _, _ = O.convert(cp, O.convert_16u_to_32f(ref_mm)); cc, _, _ = O.convert(cp, O.convert_16u_to_32f(cur_mm))
        b = time.perf_counter()
        O.align(apar, cr, cc)
        c = time.perf_counter()
        t_conv += b - a; t_align += c - b; done += 1
        if time.perf_counter() - t0 > budget_s:
            break
    return done, t_conv, t_align


def _cpu_worker(job):
    """one host core: its own pairs of the same workload through the oracle, single-threaded; (pairs, seconds of oracle work)"""
    rows, cols, K, conv, alig, seeds = job
    os.environ["PWN_ORACLE_VARIANT"] = "fast"
    from g2o_frontend_amd import synth
    from oracle import oracle as O
    O.set_num_threads(1); O.set_parallel_align(False)
    cp = O.converter_params(K=K, **conv)
    apar = O.aligner_params(rows, cols, K=K, **alig)
    frames = [synth.make_pair(s, rows, cols, K) for s in seeds]
    t0 = time.perf_counter()
    for ref_mm, cur_mm, _ in frames:
        cr, _, _ = O.convert(cp, O.convert_16u_to_32f(ref_mm)); cc, _, _ = O.convert(cp, O.convert_16u_to_32f(cur_mm))
        O.align(apar, cr, cc)
    return len(frames), time.perf_counter() - t0


def cpu_baseline_child(args):
    """The CPU oracle (port of the reference CPU path; BASELINE.md §3: -O3 -march=native, built on this host) on bounded samples of the
    benchmark's own pairs: (i) one thread, (ii) OpenMP over all cores inside each alignment like the reference (rows / correspondences
    over threads, without its remainder dropping), (iii) one single-threaded process per core on independent pairs (how a CPU would
    run the loop-closure batch).  Also returns the fp64-accumulated chi2 traces of the first pairs for the bench line's chi2_match."""
    os.environ["PWN_ORACLE_VARIANT"] = "fast"
    rows, cols = args.rows, args.cols
    K, conv, alig = conf(rows, cols)
    from g2o_frontend_amd import synth
    from oracle import oracle as O
    O.lib()                                                 # builds oracle/_fast/<cpu>/libpwn_oracle.so on first use (untimed)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    # the cpus this process may be scheduled on are not the cpu TIME it may use: a container's cgroup quota (the one-GPU boxes: 16 of a 256-thread
    # host) bounds what any number of threads gets; more threads than the quota only add contention
    quota = host_cpu_info().get("cgroup_cpu_quota")
    if quota:
        cores = max(1, min(cores, int(round(quota))))
    cp = O.converter_params(K=K, **conv)
    apar = O.aligner_params(rows, cols, K=K, **alig)
    fast = getattr(O.lib(), "_pwn_variant", "checker") == "fast"
    out = {"unit": "alignments/s", "kind": "port",
           "build": "g++ -O3 -march=native -ffp-contract=off -fopenmp (built on this host)" if fast else "g++ -O2 -ffp-contract=off -fopenmp (checker build: the -O3 build failed on this host)"}
    # (i) one thread
    O.set_num_threads(1); O.set_parallel_align(False)
    done, t_conv, t_align = _cpu_pairs_loop(O, synth, rows, cols, K, cp, apar, range(0, 64), args.cpu_seconds)
    single = done / (t_conv + t_align)
    out.update(single_thread_value=single, single_thread_ms_convert=t_conv / done * 1e3, single_thread_ms_align=t_align / done * 1e3,
               align_only_single_thread_value=done / t_align)
    # (ii) OpenMP inside each alignment
    omp_cores = min(cores, 64)
    O.set_num_threads(omp_cores); O.set_parallel_align(True)
    d2, c2, a2 = _cpu_pairs_loop(O, synth, rows, cols, K, cp, apar, range(64, 192), args.cpu_seconds / 2)
    out.update(openmp_value=d2 / (c2 + a2), openmp_cores=omp_cores)
    # (iii) one process per core
    O.set_num_threads(1); O.set_parallel_align(False)
    per_core = 0
    try:
        import concurrent.futures as cf
        import multiprocessing as mp
        pc = max(1, min(cores, 64))
        per_core = max(1, int(0.5 * args.cpu_seconds * single))
        jobs = [(rows, cols, K, conv, alig, [1000 + c * per_core + i for i in range(per_core)]) for c in range(pc)]
        with cf.ProcessPoolExecutor(max_workers=pc, mp_context=mp.get_context("spawn")) as ex:
            res = list(ex.map(_cpu_worker, jobs))
        pairs = sum(r[0] for r in res); slowest = max(r[1] for r in res)
        out.update(all_cores_value=pairs / slowest, all_cores=pc)
    except Exception as e:      # never let one leg break the line
        out.update(all_cores_value=None, all_cores=0, all_cores_error=str(e)[:200])
    # the reported baseline = the strongest CPU configuration measured
    best = max([(single, 1, "one thread"), (out["openmp_value"], omp_cores, "OpenMP inside each alignment"),
                (out.get("all_cores_value") or 0.0, out.get("all_cores") or 0, "one single-threaded process per core")], key=lambda t: t[0])
    out.update(value=best[0], cores=best[1],
               sample=f"{best[2]}; {rows}x{cols} pairs of the benchmark (convert 2 frames + align, 10 GN it.), "
                      f"{done} pairs 1-thread / {d2} OpenMP / {out.get('all_cores', 0)}x{per_core if out.get('all_cores') else 0} per-core")
    # chi2 traces for chi2_match: fp64-accumulated sums (what the 1e-5 bar is stated against), canonical one-thread align loops
    O.set_num_threads(omp_cores); O.set_parallel_align(False)
    ap64 = O.aligner_params(rows, cols, K=K, accumulate_fp64=1, **alig)
    traces = []
    for s in range(0, 3):
        ref_mm, cur_mm, _ = synth.make_pair(s, rows, cols, K)
        cr, _, _ = O.convert(cp, O.convert_16u_to_32f(ref_mm)); cc, _, _ = O.convert(cp, O.convert_16u_to_32f(cur_mm))
        r64 = O.align(ap64, cr, cc, images=True)
        r32 = O.align(apar, cr, cc)
        import zlib
        traces.append({"seed": s, "chi2_fp64": [float(it["chi2_fp64"]) for it in r64["iterations"]],
                       "chi2_fp32_serial": [float(it["chi2"]) for it in r32["iterations"]], "T": r64["T"].astype(float).tolist(),
                       "T_before": [it["T_before"].astype(float).tolist() for it in r64["iterations"]],
                       "counters": [[int(it["K"]), int(it["C"]), int(it["inliers"])] for it in r64["iterations"]],
                       # the finder's index images of the last outer iteration (the bit-exact contract of the projector)
                       "index_crc": [zlib.crc32(np.ascontiguousarray(r64["ref_index"]).tobytes()), zlib.crc32(np.ascontiguousarray(r64["cur_index"]).tobytes())]})
    out["chi2_traces"] = traces
    print(json.dumps(out))


# ------------------------------------------------------------------------------------------------ the batch workload (headline, config 5)
STAGES = ["u16_to_f32", "unproject", "integral", "integral_rows", "integral_cols", "stats", "project_cur", "project_ref", "corr_linearize", "solve"]


def align_bytes(N, n_it, res, proj_cur_per_pair, proj_ref_per_pair, depth_bytes=2.0):
    """algorithmic bytes per pair from the counters the kernels emit; res: structured result array.
    depth_bytes: bytes per pixel of the frames the converter reads -- SURVEY's 8N + 64M per frame is 4N of float depth in + 4N of index image out;
    the benchmark's frames are uint16 millimetres (2N in: 6N + 64M per frame).  Until round 5 the line charged 4N for them."""
    N = float(N)
    Mr = res["n_reference"].astype(np.float64); Mc = res["n_current"].astype(np.float64)
    Ks = res["iter_candidates"].sum(1).astype(np.float64); Cs = res["iter_correspondences"].sum(1).astype(np.float64)
    convert = 2 * (depth_bytes + 4.0) * N + 64.0 * (Mr + Mc)                   # two frames: (depth in + 4N index out) + 64M each
    fused = n_it * 8.0 * N + 72.0 * Ks + 28.0 * Cs                             # all iterations
    project = proj_cur_per_pair * (16.0 * Mc + 4.0 * N) + proj_ref_per_pair * (16.0 * Mr + 4.0 * N)      # EXECUTED projections only
    align = project + fused + 8.0 * N
    return dict(convert=convert, fused=fused, project=project, align=align, Mr=Mr, Mc=Mc, Ks=Ks, Cs=Cs)


class BatchWorkload:
    """`P` pairs of one frame size on one context: convert 2P frames + align P pairs per step."""

    def __init__(self, args, device, rows, cols, P, frames_mm, seeds, use_dist, world):
        import ctypes as C
        import torch
        from g2o_frontend_amd import api, shard
        self.args, self.rows, self.cols, self.P, self.seeds, self.use_dist, self.world = args, rows, cols, P, list(seeds), use_dist, world
        self.Pmax = P                     # rows every rank contributes to the all-gather (the largest shard; set by main() in strong-scaling mode)
        self.total = world * P            # pairs of the whole job
        self.N = rows * cols
        self.K, self.conv, self.alig = conf(rows, cols)
        self.n_it = self.alig["outer_iterations"] * self.alig["inner_iterations"]
        slots = max(2, args.streams) * max(args.sub_frames, args.sub_pairs, 1)      # room for one sub-batch in flight per stream
        self.ctx = api.Context(device=device, max_rows=rows, max_cols=cols, max_batch=slots, omega_storage=getattr(args, "omega_storage", "exact9"))
        self.ctx.set_subbatch(args.sub_frames, args.sub_pairs)
        self.converter, self.aligner = build_objects(self.ctx, rows, cols, self.K, self.conv, self.alig)
        self.frames_mm = frames_mm
        self.ref_dev = [torch.from_numpy(f[0].view(np.int16)).cuda() for f in frames_mm]
        self.cur_dev = [torch.from_numpy(f[1].view(np.int16)).cuda() for f in frames_mm]
        self.refs = [api.Cloud(self.ctx, self.N) for _ in range(P)]
        self.curs = [api.Cloud(self.ctx, self.N) for _ in range(P)]
        dev = torch.device("cuda", device)
        # two record buffers: step k+1 packs into one while step k's all-gather may still read the other
        self.records2 = [torch.empty((P, shard.RECORD_FLOATS), dtype=torch.float32, device=dev) for _ in range(2)]
        self.records = self.records2[0]
        self.k = 0
        self.gstream = [torch.cuda.Stream(device=dev) for _ in range(2)] if use_dist else None
        self.ids = np.asarray(self.seeds, np.int32)                                  # global pair ids: word 19 of the records
        self.conv_prep = self.converter.batchHandles(self.refs + self.curs, self.ref_dev + self.cur_dev)
        self.align_prep = ((C.c_void_p * P)(*[c.h for c in self.refs]), (C.c_void_p * P)(*[c.h for c in self.curs]), P)
        self.step_prep = self.aligner.convertAlignHandles(self.refs, self.curs, self.ref_dev, self.cur_dev, converter=self.converter)
        self.fused = getattr(args, "step_mode", "fused") == "fused"
        self.stage_ms = {k: 0.0 for k in STAGES}; self.stage_n = {k: 0 for k in STAGES}
        self.last = {}
        self.gathered = None
        self._in_step = False
        self.inside = use_dist and not getattr(args, "gather_after_call", False)
        self.cb_s = 0.0; self.call_s = 0.0
        if self.inside:
            self.ctx.set_enqueued_callback(self._queue_gather)

    def _queue_gather(self):
        """inside the step's (last) library call, after its device work is queued and before it waits (pwn_hip_ctx_set_enqueued_callback): the
        all-gather of this step's records is queued behind the call's own stream (pwn_hip_ctx_signal_stream), so that neither its enqueue nor its
        latency sits between two steps"""
        import torch
        from g2o_frontend_amd import shard
        if not self._in_step:              # another call on this context (the extra lines of a forced one-rank run): not a step, nothing to gather
            return
        t0 = time.perf_counter()
        gs = self.gstream[self.k % 2]
        with torch.cuda.stream(gs):
            self.ctx.signal_stream(gs)
            self.gathered = shard.gather_records(self.records2[self.k % 2], self.world, self.Pmax, force=True)      # the only collective of the path
        self.cb_s += time.perf_counter() - t0

    def step(self, profile=False):
        """one pass of the hot path over the rank's pairs; the 256-byte result records are written by a kernel straight into the device tensor the
        all-gather sends (no trip through the host), the caller's own copy of the results comes back beside them"""
        from g2o_frontend_amd import shard
        rec = self.records2[self.k % 2]
        self._in_step = True
        if self.use_dist:
            # k_pack_records writes this buffer on the library's own stream; the all-gather of step k-2 read it on gstream[k % 2]: the context's
            # work of this step is ordered after what that stream holds (pwn_hip_ctx_wait_stream)
            self.ctx.wait_stream(self.gstream[self.k % 2])
        tcall = time.perf_counter()
        if self.fused:
            res = self.aligner.convertAlignBatch(self.converter, None, None, None, None, raw_scale=0.001, records=rec, pair_ids=self.ids,
                                                 prepared=self.step_prep)
            if profile:
                for k in STAGES:
                    ms, n = self.ctx.stage_ms(k); self.stage_ms[k] += ms; self.stage_n[k] += n
        else:
            self.converter.computeBatch(self.refs + self.curs, self.ref_dev + self.cur_dev, raw_scale=0.001, prepared=self.conv_prep)
            if profile:
                for k in STAGES[:6]:
                    ms, n = self.ctx.stage_ms(k); self.stage_ms[k] += ms; self.stage_n[k] += n
            res = self.aligner.alignBatchRecords(None, None, rec, pair_ids=self.ids, prepared=self.align_prep)
            if profile:
                for k in STAGES[6:]:
                    ms, n = self.ctx.stage_ms(k); self.stage_ms[k] += ms; self.stage_n[k] += n
        self.call_s += time.perf_counter() - tcall
        if self.inside:
            self.ctx.take_callback_error()
            self.last["gathered"] = self.gathered                                      # queued from inside the call (_queue_gather)
        elif self.use_dist:
            import torch
            with torch.cuda.stream(self.gstream[self.k % 2]):                          # after the call has returned: its records are complete
                self.last["gathered"] = shard.gather_records(rec, self.world, self.Pmax, force=True)
        else:
            self.last["gathered"] = shard.gather_records(rec, self.world, self.Pmax, force=False)
        self.k += 1
        self._in_step = False
        self.last["res"] = res

    def barrier(self):
        import torch
        if self.use_dist:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    def run(self, steps, warmup, profile=True):
        """timed region in the product configuration (streams, no instrumentation), then the same steps again on one stream with a
        hipEvent pair around every kernel stage: with two streams the launches of different sub-batches overlap, so a launch's elapsed
        time is not the kernel's own duration (the rocprofv3 summaries in profiles/ are taken the same way: bench.py --streams 1)."""
        ctx = self.ctx
        ctx.set_concurrency(self.args.streams); ctx.set_profiling(False)
        for _ in range(warmup):
            self.step()
        self.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        self.barrier()
        dt = time.perf_counter() - t0
        if getattr(self.args, "dump_outputs", None):
            # what the last timed step returned, before the profiled pass and the extra lines overwrite the record buffers (--dump-outputs)
            self.timed_last = {"res": self.last["res"], "gathered": self.last["gathered"].cpu().numpy().copy()}
        dt_serial = None
        if profile:
            ctx.set_concurrency(1); ctx.set_profiling(True)
            self.step()
            self.barrier()
            t1 = time.perf_counter()
            for _ in range(steps):
                self.step(True)
            self.barrier()
            dt_serial = time.perf_counter() - t1
            ctx.set_profiling(False); ctx.set_concurrency(self.args.streams)
        return dt, dt_serial

    def time_collectives(self, n=20):
        """the all-gather of the records alone (no compute): ms per call"""
        import torch
        from g2o_frontend_amd import shard
        if not self.use_dist:
            return {}
        self.barrier(); t0 = time.perf_counter()
        for _ in range(n):
            shard.gather_records(self.records, self.world, self.Pmax, force=True)
        torch.cuda.synchronize()
        return {"gather_ms": (time.perf_counter() - t0) / n * 1e3}

    # ---- algorithmic bytes of SURVEY.md §8(d) from the measured counters
    def bytes_per_pair(self, res, proj_cur_per_pair, proj_ref_per_pair):
        return align_bytes(self.N, self.n_it, res, proj_cur_per_pair, proj_ref_per_pair)

    def report(self, steps, dt, dt_serial, world):
        res = self.last["res"]; P = self.P
        # sub-batches a step was executed in (the library balances them over the streams): every sub-batch launches the fused pass n_it times
        nsub = max(1.0, self.stage_n["corr_linearize"] / max(steps, 1) / max(self.n_it, 1)) if dt_serial else 1.0
        pc = self.stage_n["project_cur"] / max(steps, 1) / nsub if dt_serial else 1.0
        pr = self.stage_n["project_ref"] / max(steps, 1) / nsub if dt_serial else float(self.n_it)
        b = self.bytes_per_pair(res, pc, pr)
        total_step = float((b["convert"] + b["align"]).sum())
        launches = max(self.stage_n["corr_linearize"], 1)
        k_ms = self.stage_ms["corr_linearize"] / launches
        k_bytes = float(b["fused"].sum()) * steps / launches
        achieved = k_bytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
        conv_ms = sum(self.stage_ms[k] for k in STAGES[:6]) / max(steps, 1)
        conv_GBps = float(b["convert"].sum()) / (conv_ms * 1e-3) / 1e9 if conv_ms > 0 else 0.0
        # HBM traffic per launch from the PMC passes committed under profiles/ (tools/summarize_pmc.py writes profiles/traffic.json from the newest
        # summary; its `version` travels with the line).  Every term of every kernel's traffic is per pixel / per point, so other frame sizes and
        # launch sizes scale with pixels x items per launch.
        traffic = None; tj = {}
        tfile = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tfile):
            try:
                tj = json.load(open(tfile))
            except Exception:
                tj = {}

        # a table measured at this very frame size (profiles/traffic.json: "sizes") is used as it is; otherwise the VGA table scaled by pixels
        tsz = tj.get("sizes", {}).get(f"{self.rows}x{self.cols}")
        tuse = tsz if tsz else tj

        def pmc_bytes(kernel, items_per_launch):
            e = tuse.get("kernels", {}).get(kernel)
            if not e:
                return None
            return e["bytes_per_launch"] / e.get("items_per_launch", tuse.get("items_per_launch", 64)) * (self.N / tuse.get("pixels_per_frame", 307200)) * items_per_launch
        traffic = pmc_bytes("k_corr_linearize", P * self.n_it * steps / launches)
        # the other kernels of the step, each against the same peak: algorithmic bytes of its share of SURVEY.md 8(d)'s formulas / its own
        # average launch time (hipEvent pairs of the serial profiled pass), PMC traffic beside it
        F = 2 * P                                                      # frames per step
        Msum = float(b["Mr"].sum() + b["Mc"].sum())
        per_kernel = {}

        def kernel_entry(name, stage, alg_bytes_per_step, items_per_step, note):
            n = self.stage_n[stage]
            if not n or self.stage_ms[stage] <= 0:
                return
            ms = self.stage_ms[stage] / n
            alg = alg_bytes_per_step * steps / n
            tr = pmc_bytes(name, items_per_step * steps / n)
            ach = alg / (ms * 1e-3) / 1e9
            per_kernel[name] = {"achieved": ach, "frac": ach / HBM_PEAK_GBS, "unit": "GB/s", "avg_launch_ms": ms, "launches": n,
                                "bytes_per_launch_algorithmic": alg, "traffic": tr,
                                "traffic_over_algorithmic": (tr / alg) if tr else None,
                                "traffic_GBps": (tr / (ms * 1e-3) / 1e9) if tr else None, "algorithmic_bytes": note}
        kernel_entry("k_stats", "stats", 6.0 * self.N * F + 64.0 * Msum, F, "2N depth + 4N index in, 64M cloud out per frame (the 40N integral planes are a temporary)")
        kernel_entry("k_unproject_integral", "integral", 6.0 * self.N * F, F, "2N depth in, 4N index out per frame (the 40N integral planes are a temporary)")
        npj = self.stage_n["project_cur"] + self.stage_n["project_ref"]
        if npj:
            self.stage_ms["project"] = self.stage_ms["project_cur"] + self.stage_ms["project_ref"]; self.stage_n["project"] = npj
            kernel_entry("k_project", "project", float(b["project"].sum()), P * (pc + pr), "16M + 4N per executed projection")
        dom = max(STAGES, key=lambda k: self.stage_ms[k])
        roofline = {"bound": "hbm", "kernel": "k_corr_linearize", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                    "traffic_over_algorithmic": (traffic / k_bytes) if (traffic and k_bytes) else None,
                    "traffic_source": {"file": "profiles/traffic.json", "version": tuse.get("version"), "pmc_summary": tuse.get("source"),
                                       "measured_at_this_frame_size": bool(tsz) or (self.rows, self.cols) == (480, 640)},
                    "bytes_per_launch_algorithmic": k_bytes, "avg_launch_ms": k_ms, "launches": self.stage_n["corr_linearize"],
                    "dominant_by_time": dom,
                    "traffic_GBps": (traffic / (k_ms * 1e-3) / 1e9) if (traffic and k_ms > 0) else None,
                    # the whole step (timed region, product configuration) and the converter (serial profiled pass) against the same peak
                    "path_achieved_GBps": total_step * steps / dt / 1e9, "path_frac": total_step * steps / dt / 1e9 / HBM_PEAK_GBS,
                    "converter_ms_per_step": conv_ms, "converter_achieved_GBps": conv_GBps, "converter_frac": conv_GBps / HBM_PEAK_GBS,
                    "projections_per_pair": pc + pr,
                    "other_kernels": per_kernel,
                    "measured_in": "serial profiled pass of the same K steps (one stream, hipEvent pair per kernel stage); "
                                   "the timed region runs the streams without instrumentation",
                    "serial_pass_alignments_per_s": (self.total * steps / dt_serial) if dt_serial else None}
        return dict(value=self.total * steps / dt, ms_per_step=dt / steps * 1e3, roofline=roofline,
                    path_roofline={"algorithmic_bytes_per_pair": total_step / P, "convert_bytes_per_pair": float(b["convert"].sum()) / P,
                                   "depth_bytes_per_pixel_charged": 2.0, "achieved_GBps": total_step * steps / dt / 1e9,
                                   "frac_of_peak": total_step * steps / dt / 1e9 / HBM_PEAK_GBS,
                                   "projections_counted_per_pair": pc + pr},
                    stage_ms_per_step={k: self.stage_ms[k] / max(steps, 1) for k in STAGES},
                    stage_launches_per_step={k: self.stage_n[k] / max(steps, 1) for k in STAGES},
                    counters_mean={"M_ref": float(b["Mr"].mean()), "M_cur": float(b["Mc"].mean()), "K_sum": float(b["Ks"].mean()),
                                   "C_sum": float(b["Cs"].mean()), "chi2_final": float(res["error"].mean()), "inliers_final": float(res["inliers"].mean())})

    def close(self):
        self.ctx.set_enqueued_callback(None)
        self.refs = self.curs = None
        self.ctx.close()


# ------------------------------------------------------------------------------------------------ processPartition workload (--mode partition)
PARTITION_SCENE = 7          # seed of the scene every frame of the partition workload looks at
PARTITION_POSE0 = 5000       # other frame k: camera pose synth.pair_pose(PARTITION_POSE0 + k) relative to `current` (<= 5 cm, ~2.3 deg per axis)


def partition_jobs(ids, rows, cols, K):
    """render jobs of the `other` frames with global ids `ids` (views of one scene from poses around `current`'s)"""
    from g2o_frontend_amd import synth
    return [("frame", PARTITION_SCENE, synth.pair_pose(PARTITION_POSE0 + k).tolist(), rows, cols, K, 1 + k) for k in ids]


def partition_guesses(ids, t_noise=0.01, q_noise=0.004):
    """iT * other.T of PwnCloser::processPartition (pwn_tracker/pwn_closer.cpp:101): the odometry's estimate of the pose of `other` in `current`'s
    frame = the true relative pose disturbed by a seeded error of <= 1 cm / ~0.5 deg per axis.  [n, 4, 4] float64 (matchClouds zeroes the z translation)."""
    from g2o_frontend_amd import synth
    out = []
    for k in ids:
        u = synth._uniform(PARTITION_POSE0 + k, 7, 6)
        dv = np.concatenate([(2 * u[0:3] - 1) * t_noise, (2 * u[3:6] - 1) * q_noise])
        out.append(synth.pair_pose(PARTITION_POSE0 + k) @ synth.v2t(dv))
    return out


def pp_owner(j, world):
    """pipelined processPartition: the rank that converts, exports and broadcasts keyframe j"""
    return j % world


def pp_ctrl_row(owner, rows_per_rank):
    """row of the gathered record tensor that holds `owner`'s control row (the last row of its block)"""
    return owner * rows_per_rank + rows_per_rank - 1


def simulate_partition_pipeline_cpu(rank, world, steps, dist):
    """The bookkeeping of PartitionWorkload's pipelined step with nothing but host tensors and gloo (tests: world 3 and 8 on the CPU) and flat clouds whose
    SIZE DIFFERS from keyframe to keyframe -- which the GPU benchmark, re-using one `current` frame, never exercises: the ring of four flat buffers, the owner
    rotation, the size that travels one step ahead in the owner's control row, the broadcast of exactly the bytes written, the import into the replica the
    NEXT step matches against.  Returns True when every step on this rank matched against the keyframe it should have, with the bytes its owner made."""
    import torch
    R, rows = 4, 5                                             # ring; rows per rank in the record tensor (4 records + the control row)

    def payload(j):                                            # the flat form of keyframe j: a multiple of 256 bytes, another length for every j
        n = 256 * (40 + (j * 37) % 23)
        return ((np.arange(n, dtype=np.uint64) * 2654435761 + 97 * j) % 251).astype(np.uint8)
    bound = 256 * 64
    flat = [torch.zeros(bound, dtype=torch.uint8) for _ in range(R)]
    size = [0] * R
    rep_key = [-1, -1]                                         # which keyframe each replica holds
    ok = True

    def convert_export(j):                                     # the look-ahead job of keyframe j on its owner
        p = payload(j)
        flat[j % R][: p.size] = torch.from_numpy(p)
        return int(p.size)

    def bcast(t, src):
        if world > 1:
            dist.broadcast(t, src=src)

    def import_(j):                                            # what arrived must be what keyframe j's owner made, byte for byte
        nonlocal ok
        got = flat[j % R][: size[j % R]].numpy()
        ok = ok and size[j % R] == payload(j).size and np.array_equal(got, payload(j))
        rep_key[j % 2] = j
    # prime
    for j in (0, 1, 2):
        n = torch.zeros(1, dtype=torch.int64)
        if rank == pp_owner(j, world):
            n[0] = convert_export(j)
        bcast(n, pp_owner(j, world)); size[j] = int(n.item())
    bcast(flat[0][: size[0]], pp_owner(0, world)); import_(0)
    bcast(flat[1][: size[1]], pp_owner(1, world))               # (asynchronous on the GPU: imported inside step 0's call)
    pending = None
    if rank == pp_owner(3, world):
        pending = (3, convert_export(3))
    ctrl_prev = None
    for k in range(steps):
        ok = ok and rep_key[k % 2] == k                         # the step's matches run against keyframe k
        rec = torch.full((rows, 72), -1.0)
        rec[: rows - 1, 19] = torch.arange(rows - 1, dtype=torch.float32) + rank * (rows - 1)      # four records of this rank
        # ---- what _overlap() does inside the match call
        if rank == pp_owner(k + 3, world):
            ok = ok and pending is not None and pending[0] == k + 3
            rec[rows - 1, 0] = float(pending[1] // 256); pending = None
        if rank == pp_owner(k + 4, world):
            pending = (k + 4, convert_export(k + 4))            # buffer k % 4: keyframe k was imported during step k-1
        if k >= 1:
            size[(k + 2) % R] = ctrl_prev
        bcast(flat[(k + 2) % R][: size[(k + 2) % R]], pp_owner(k + 2, world))
        g = torch.empty((world * rows, 72))
        if world > 1:
            dist.all_gather(list(g.view(world, rows, 72).unbind(0)), rec)
        else:
            g = rec
        ctrl_prev = int(g[pp_ctrl_row(pp_owner(k + 3, world), rows), 0].item()) * 256      # the size of keyframe k+3, for step k+1's broadcast
        ok = ok and sorted(int(x) for x in g[:, 19].tolist() if x >= 0) == list(range(world * (rows - 1)))
        import_(k + 1)
    return bool(ok)


class PartitionWorkload:
    """PwnCloser::processPartition (pwn_tracker/pwn_closer.cpp:85-111) sharded over the GPUs of a node (Partitioning): the clouds of the
    other partition stay on the GPU that converted them (PwnCache: pwn_tracker_cache.cpp:24-51), the cloud of `current` is converted on rank 0 and
    replicated with ONE broadcast of its flat form (pwn_hip_cloud_export / _import), every rank runs matchFrames' data path (matchClouds:
    align from the odometry guess with the z translation zeroed + depth-agreement score, pwn_matcher_base.cpp:88-183) of `current` against its
    shard, and the 288-byte match records are all-gathered.  `current` is the aligner's REFERENCE cloud of every pair (matchFrames(current, other):
    from = current, pwn_closer.cpp:102,128-133).

    Pipelined (the default).  The reference's outer loop hands the closer one `current` keyframe after the other, and nothing keyframe k's matches
    produce is needed to make the cloud of keyframe k+1.  A step is ONE library call -- the matches of keyframe k against the shard -- and everything
    else the step needs is queued from inside that call, after its device work has been queued and before it waits (pwn_hip_ctx_set_enqueued_callback),
    so the host's share runs while the device works:
      * rank 0: the helper job that converted keyframe k+3 and wrote its flat form is collected, the job for keyframe k+4 started
        (pwn_hip_convert_export_begin / _end; flat buffers form a ring of four);
      * keyframe k+2's flat form is broadcast on a side stream -- only the bytes written; their count reached every rank in the control row of
        step k-1's record all-gather;
      * the all-gather of step k's records is queued behind the call's own stream (pwn_hip_ctx_signal_stream), carrying the size of keyframe k+3;
      * replica (k+1) % 2 is imported from keyframe k+1's flat form (broadcast during step k-1) through a second, small context, next to the matches.
    Without RCCL (one rank, plain run) the helper converts keyframe k+2 straight into a third replica.
    --partition-serial: round 5's chain (convert, export, broadcast of the buffer's bound, import, match), kept for the A/B."""

    RING = 4

    def __init__(self, args, device, rows, cols, ids, other_frames_mm, current_mm, use_dist, world, rank, total):
        import torch
        from g2o_frontend_amd import api
        self.args, self.rows, self.cols, self.ids, self.use_dist, self.world, self.rank, self.total = args, rows, cols, list(ids), use_dist, world, rank, total
        self.P = len(self.ids); self.Pmax = (total + world - 1) // world
        self.N = rows * cols
        self.K, self.conv, self.alig = conf(rows, cols)
        self.n_it = self.alig["outer_iterations"] * self.alig["inner_iterations"]
        slots = max(2, args.streams) * max(args.sub_frames, args.sub_pairs, 1)
        self.ctx = api.Context(device=device, max_rows=rows, max_cols=cols, max_batch=slots, omega_storage=args.omega_storage)
        self.ctx.set_subbatch(args.sub_frames, args.sub_pairs)
        self.converter, self.aligner = build_objects(self.ctx, rows, cols, self.K, self.conv, self.alig)
        alproj = api.PinholePointProjector(); alproj.setMinDistance(self.alig["min_distance"]); alproj.setMaxDistance(self.alig["max_distance"])
        self.aligner.setProjector(alproj)                 # matchClouds re-configures the aligner's projector on every call (pwn_matcher_base.cpp:117-119)
        self.matcher = api.PwnMatcherBase(self.aligner, self.converter); self.matcher.setScale(1)
        self.Km = np.array([[self.K[0], 0, self.K[2]], [0, self.K[1], self.K[3]], [0, 0, 1]], np.float32)
        self.I = np.eye(4, dtype=np.float32)
        dev = torch.device("cuda", device)                # the context's device, whatever torch's current device is
        # the cache of the other partition: this rank's shard, converted once (untimed)
        self.other_dev = [torch.from_numpy(f.view(np.int16)).to(dev) for f in other_frames_mm]
        self.others = [api.Cloud(self.ctx, self.N) for _ in range(self.P)]
        if self.P:
            self.converter.computeBatch(self.others, self.other_dev, raw_scale=0.001)
        self.other_dev = None
        self.pipeline = not getattr(args, "partition_serial", False)
        # pipelined: the look-ahead work ROTATES over the ranks (keyframe j is converted, exported and broadcast by rank j % world), so that no rank's step is
        # longer than the others' by a conversion -- every rank holds the raw `current` frames it will own.  Serial chain: rank 0 does it all.
        self.cur_dev = torch.from_numpy(current_mm.view(np.int16)).to(dev) if (rank == 0 or self.pipeline) else None
        # rank 0 of a forced one-rank run takes the replica path too (export -> broadcast -> import), so that the byte path is exercised
        self.roundtrip = use_dist and world == 1
        bound = api.Cloud.flatBound(self.N, args.omega_storage, self.N)
        # rows [0:P] the records k_pack_records writes, [P:Pmax] padding, row Pmax the rank's control row (pair id -1 like padding: assemble() drops it)
        # two of them: step k+1 packs its records while step k's all-gather may still be reading
        self.records2 = [torch.full((self.Pmax + 1, api.MATCH_RECORD_FLOATS), -1.0, dtype=torch.float32, device=dev) for _ in range(2)]
        self.records = self.records2[0]
        self.ids_np = np.asarray(self.ids, np.int32)
        self.guesses = partition_guesses(self.ids)
        self.stage_ms = {k: 0.0 for k in STAGES + ["match_score"]}; self.stage_n = {k: 0 for k in STAGES + ["match_score"]}
        self.flat_bytes = 0
        self.rank0_only_host_s = 0.0; self.rank0_job_ms = 0.0; self.import_host_s = 0.0; self.steps_done = 0
        self.phase_s = {k: 0.0 for k in ("step", "match_call", "inside_callback")}      # host clock per step: the whole step, the library call, the callback inside it
        self.last = {}; self.io = None; self.ticket = None; self.k = 0
        if self.pipeline:
            if use_dist:
                self.io = api.Context(device=device, max_rows=rows, max_cols=cols, max_batch=1, omega_storage=args.omega_storage)      # imports run here, next to the matches
                self.rep = [api.Cloud(self.io, self.N) for _ in range(2)]
                self.flat = [torch.empty(bound, dtype=torch.uint8, device=dev) for _ in range(self.RING)]
                self.conv_cloud = api.Cloud(self.ctx, self.N)      # what the helper converts into before it exports (on the rank that owns the keyframe)
                self.side = torch.cuda.Stream(device=dev); self.imp_stream = torch.cuda.Stream(device=dev)
                self.gstream = [torch.cuda.Stream(device=dev) for _ in range(2)]      # the all-gathers alternate between two streams: step k+1 waits for step k-1's only
                self.ctrl_send = [torch.zeros(4, dtype=torch.float32).pin_memory() for _ in range(2)]
                self.ctrl_host = [torch.zeros(4, dtype=torch.float32).pin_memory() for _ in range(2)]
                self.ctrl_ev = [torch.cuda.Event() for _ in range(2)]
                self.size = [0] * self.RING; self.bw = [None] * self.RING
            else:
                self.rep = [api.Cloud(self.ctx, self.N) for _ in range(3)]
                self.flat = [None]
                self.conv_cloud = None
            self.prep = [self.matcher.matchHandles([c] * self.P, self.others, self.guesses) for c in self.rep]
            self._prime()
            self.ctx.set_enqueued_callback(self._overlap)
        else:
            self.current = api.Cloud(self.ctx, self.N)        # rank 0: what the converter fills; other ranks: the replica the broadcast fills
            self.replica = api.Cloud(self.ctx, self.N) if self.roundtrip else None
            self.flat = [torch.empty(bound, dtype=torch.uint8, device=dev)]
            ref = self.replica if self.roundtrip else self.current
            self.prep = [self.matcher.matchHandles([ref] * self.P, self.others, self.guesses)]

    def _collect(self, keys):
        for k in keys:
            ms, n = self.ctx.stage_ms(k); self.stage_ms[k] += ms; self.stage_n[k] += n

    def _prime(self):
        """fills the pipeline (untimed).  RCCL: keyframes 0-2 converted and exported, their sizes known everywhere; keyframe 0 in replica 0 on every
        rank, keyframe 1's broadcast in flight, keyframe 3's job running.  Plain: keyframe 0 in replica 0, keyframe 1's job running."""
        import torch
        import torch.distributed as dist
        cv = self.converter
        if not self.use_dist:
            cv.computeExportEnd(cv.computeExportBegin(self.rep[0], self.cur_dev))
            self.ticket = cv.computeExportBegin(self.rep[1], self.cur_dev)
            return
        own = self.owner
        for j in (0, 1, 2):
            n = torch.zeros(1, dtype=torch.int64, device=self.records.device)
            if self.rank == own(j):
                w, _ = cv.computeExportEnd(cv.computeExportBegin(self.conv_cloud, self.cur_dev, flat=self.flat[j]))
                n[0] = w
            dist.broadcast(n, src=own(j))
            self.size[j] = int(n.item())
        dist.broadcast(self.flat[0][: self.size[0]], src=own(0))
        self.io.wait_stream()
        self.rep[0].importFlat(self.flat[0][: self.size[0]])
        self.flat_bytes = self.size[0]
        with torch.cuda.stream(self.side):
            self.bw[1] = dist.broadcast(self.flat[1][: self.size[1]], src=own(1), async_op=True)
        if self.rank == own(3):
            self.ticket = cv.computeExportBegin(self.conv_cloud, self.cur_dev, flat=self.flat[3])

    def owner(self, j):
        """the rank that converts, exports and broadcasts keyframe j"""
        return pp_owner(j, self.world)

    def _overlap(self):
        """runs inside step k's match call, after its device work is queued and before it waits"""
        import torch
        import torch.distributed as dist
        from g2o_frontend_amd import shard
        tc = time.perf_counter()
        cv = self.converter; k = self.k; R = self.RING
        if not self.use_dist:
            w, ms = cv.computeExportEnd(self.ticket)                                  # keyframe k+1 sits in replica (k+1) % 3
            self.rank0_job_ms += ms
            self.ticket = cv.computeExportBegin(self.rep[(k + 2) % 3], self.cur_dev)      # keyframe k+2 -> the replica step k-1 matched against
            self.rank0_only_host_s += time.perf_counter() - tc
            self.gathered = shard.gather_records(self.records2[k % 2], self.world, self.Pmax + 1, force=False)
            self.phase_s["inside_callback"] += time.perf_counter() - tc
            return
        own = self.owner
        if self.rank == own(k + 3):
            w, ms = cv.computeExportEnd(self.ticket); self.ticket = None              # keyframe k+3's flat form is in buffer (k+3) % 4 of its owner
            self.rank0_job_ms += ms
            cs = self.ctrl_send[k % 2]; cs[0] = float(w // 256)                        # its size rides in the owner's control row of this step's all-gather
        if self.rank == own(k + 4):
            self.ticket = cv.computeExportBegin(self.conv_cloud, self.cur_dev, flat=self.flat[(k + 4) % R])      # buffer k % 4: imported during step k-1
        if self.rank in (own(k + 3), own(k + 4)):
            self.rank0_only_host_s += time.perf_counter() - tc
        if k >= 1:                                                                   # size of keyframe k+2: control row of step k-1's all-gather
            self.ctrl_ev[(k - 1) % 2].synchronize()
            self.size[(k + 2) % R] = int(self.ctrl_host[(k - 1) % 2][0].item()) * 256
        j2 = (k + 2) % R
        with torch.cuda.stream(self.side):                                           # keyframe k+2 travels while keyframe k is matched; only the bytes written
            self.bw[j2] = dist.broadcast(self.flat[j2][: self.size[j2]], src=own(k + 2), async_op=True)
        gs = self.gstream[k % 2]; rec = self.records2[k % 2]
        with torch.cuda.stream(gs):
            if self.rank == own(k + 3):
                rec[self.Pmax, :4].copy_(self.ctrl_send[k % 2], non_blocking=True)
            self.ctx.signal_stream(gs)                                               # the gather's stream continues after this call's records are packed
            self.gathered = shard.gather_records(rec, self.world, self.Pmax + 1, force=True)      # the records + one control row per rank
            self.ctrl_host[k % 2].copy_(self.gathered[pp_ctrl_row(own(k + 3), self.Pmax + 1), :4], non_blocking=True)   # its owner's control row: the size of keyframe k+3
            self.ctrl_ev[k % 2].record(gs)
        ti = time.perf_counter()
        j1 = (k + 1) % R
        with torch.cuda.stream(self.imp_stream):
            self.bw[j1].wait()                                                       # keyframe k+1's broadcast (queued during step k-1)
        self.io.wait_stream(self.imp_stream)
        self.rep[(k + 1) % 2].importFlat(self.flat[j1][: self.size[j1]])              # on the small context: waits for the broadcast and its own copies only
        self.flat_bytes = self.size[j1]
        self.import_host_s += time.perf_counter() - ti
        self.phase_s["inside_callback"] += time.perf_counter() - tc

    def step(self, profile=False):
        if not self.pipeline:
            return self._step_serial(profile)
        t0 = time.perf_counter()
        nrep = len(self.rep)
        rec = self.records2[self.k % 2]
        if self.use_dist:
            self.ctx.wait_stream(self.gstream[self.k % 2])      # this records buffer is free again: step k-2's all-gather read it on that stream
        res = None
        t1 = time.perf_counter()
        res = self.matcher.matchCloudsBatchRecords(None, None, self.I, self.I, self.Km, self.rows, self.cols, rec[: self.P], pair_ids=self.ids_np,
                                                   prepared=self.prep[self.k % nrep])
        self.phase_s["match_call"] += time.perf_counter() - t1
        self.ctx.take_callback_error()
        if profile:
            self._collect(STAGES[6:] + ["match_score"])
        self.k += 1; self.steps_done += 1
        self.last["gathered"] = self.gathered
        self.last["res"] = res
        self.phase_s["step"] += time.perf_counter() - t0

    def _step_serial(self, profile=False):
        import torch.distributed as dist
        from g2o_frontend_amd import shard
        if self.rank == 0:
            self.converter.computeBatch([self.current], [self.cur_dev], raw_scale=0.001)           # makeCloud of `current` (pwn_closer.cpp:92-93: _cache->get(current))
            if profile:
                self._collect(STAGES[:6])
            if self.use_dist:
                self.flat_bytes = self.current.exportFlat(self.flat[0])                            # complete on return
        if self.use_dist:
            dist.broadcast(self.flat[0], src=0)                                                   # the whole buffer (the other ranks do not know the size)
            self.ctx.wait_stream()                                                                # the import reads what the broadcast wrote; the records
            if self.rank != 0:                                                                    # buffer is free again (previous all-gather)
                self.current.importFlat(self.flat[0])
            elif self.roundtrip:
                self.replica.importFlat(self.flat[0])
        res = None
        if self.P:
            res = self.matcher.matchCloudsBatchRecords(None, None, self.I, self.I, self.Km, self.rows, self.cols, self.records[: self.P], pair_ids=self.ids_np,
                                                       prepared=self.prep[0])
            if profile:
                self._collect(STAGES[6:] + ["match_score"])
        self.steps_done += 1
        self.last["gathered"] = shard.gather_records(self.records, self.world, self.Pmax + 1, force=self.use_dist)
        self.last["res"] = res

    barrier = BatchWorkload.barrier
    run = BatchWorkload.run

    def time_collectives(self, n=20):
        """the two collectives alone (no compute): ms per broadcast of the flat cloud, ms per all-gather of the records"""
        import torch
        import torch.distributed as dist
        from g2o_frontend_amd import shard
        out = {}
        if not self.use_dist:
            return out
        self.barrier(); t0 = time.perf_counter()
        nbytes = int(self.flat_bytes) if self.pipeline else int(self.flat[0].numel())      # what a step sends: the bytes written / the buffer's bound
        scratch = torch.empty(int(self.flat[0].numel()), dtype=torch.uint8, device=self.records.device)      # not a buffer of the pipeline
        for _ in range(n):
            dist.broadcast(scratch[:nbytes], src=0)
        torch.cuda.synchronize(); out["broadcast_ms"] = (time.perf_counter() - t0) / n * 1e3
        self.barrier(); t0 = time.perf_counter()
        for _ in range(n):
            shard.gather_records(self.records, self.world, self.Pmax + 1, force=True)
        torch.cuda.synchronize(); out["gather_ms"] = (time.perf_counter() - t0) / n * 1e3
        out["broadcast_bytes"] = nbytes; out["flat_cloud_bytes"] = int(self.flat_bytes); out["flat_buffer_bound_bytes"] = int(self.flat[0].numel())
        return out

    def report(self, steps, dt, dt_serial, world):
        res, sc = self.last["res"]
        P = self.P
        r = res
        nsub = max(1.0, self.stage_n["corr_linearize"] / max(steps, 1) / max(self.n_it, 1)) if dt_serial else 1.0
        pc = self.stage_n["project_cur"] / max(steps, 1) / nsub if dt_serial else 1.0
        pr = self.stage_n["project_ref"] / max(steps, 1) / nsub if dt_serial else float(self.n_it)
        b = align_bytes(self.N, self.n_it, r, pc, pr)
        Mcur = float(r["n_reference"][0]) if P else 0.0
        step_bytes = float(b["align"].sum()) + (6.0 * self.N + 64.0 * Mcur) / max(world, 1)      # + this rank's share of the one conversion per step (u16 frame)
        # HBM traffic of the dominant kernel from the PMC passes of THIS workload (profiles/traffic.json: "modes" -> "partition"), per pair-iteration
        traffic = None; tsrc = None
        try:
            tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
            tm = tj.get("modes", {}).get("partition")
            e = tm["kernels"]["k_corr_linearize"] if tm else None
            if e and (self.rows, self.cols) == (480, 640):
                traffic = e["bytes_per_launch"] / e["items_per_launch"] * (P * self.n_it * steps / launches_of(self))
                tsrc = {"file": "profiles/traffic.json", "table": "modes.partition", "version": tm.get("version"), "pmc_summary": tm.get("source")}
        except Exception:
            traffic = None
        launches = max(self.stage_n["corr_linearize"], 1)
        k_ms = self.stage_ms["corr_linearize"] / launches
        k_bytes = float(b["fused"].sum()) * steps / launches
        achieved = k_bytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
        acc = __import__("g2o_frontend_amd.api", fromlist=["api"]).PwnCloserAcceptance()
        accepted = sum(1 for m in sc if acc.accept(dict(image_nonZeros=m.image_non_zeros, image_outliers=m.image_outliers, image_inliers=m.image_inliers)))
        from g2o_frontend_amd import synth
        terr = max(float(np.abs(r["T"][i].reshape(4, 4).T[:3, 3] - synth.pair_pose(PARTITION_POSE0 + k)[:3, 3]).max()) for i, k in enumerate(self.ids)) if P else 0.0
        nst = max(self.steps_done, 1)
        pipe = {"pipelined": bool(self.pipeline), "steps_counted": self.steps_done,
                "lookahead_rotates_over_ranks": bool(self.pipeline),      # keyframe j is converted / exported / broadcast by rank j % world: rank 0 pays the figures below every world-th step
                # host time only rank 0 spends per step: collecting the look-ahead job, the control row, starting the next job.  Pipelined: inside the
                # match call's callback, i.e. while the device works -- not on the step's critical path
                "rank0_only_host_ms_per_step": self.rank0_only_host_s / nst * 1e3,
                # the look-ahead job itself (conversion of one frame + export on the helper thread's streams), beside the matches
                "rank0_lookahead_job_ms_per_step": self.rank0_job_ms / nst,
                # every rank: wait for the next keyframe's broadcast + import of the replica (second context), inside the callback as well
                "import_host_ms_per_step": self.import_host_s / nst * 1e3,
                "host_ms_per_step": {k: v / nst * 1e3 for k, v in self.phase_s.items()},
                # what the host adds to a step outside the library call (device idle): step - match_call
                "host_ms_per_step_outside_the_call": (self.phase_s["step"] - self.phase_s["match_call"]) / nst * 1e3}
        roofline = {"bound": "hbm", "kernel": "k_corr_linearize", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                    "traffic": traffic, "traffic_over_algorithmic": (traffic / k_bytes) if (traffic and k_bytes) else None,
                    "traffic_GBps": (traffic / (k_ms * 1e-3) / 1e9) if (traffic and k_ms > 0) else None, "traffic_source": tsrc,
                    "bytes_served_by_caches": "every pair of the step gathers from the SAME `current` cloud: the algorithmic count charges its points, normals and "
                                              "information matrices once per pair, HBM delivers them about once per launch and the L2 / Infinity Cache the rest -- "
                                              "`achieved` and `frac` are algorithmic bytes on an HBM scale, `traffic` is what the counters saw",
                    "bytes_per_launch_algorithmic": k_bytes, "avg_launch_ms": k_ms, "launches": self.stage_n["corr_linearize"],
                    "path_achieved_GBps": step_bytes * world * steps / dt / 1e9, "path_frac": step_bytes * world * steps / dt / 1e9 / HBM_PEAK_GBS / max(world, 1),
                    "projections_per_pair": pc + pr,
                    "algorithmic_bytes": "per pair: executed projections (16M + 4N each) + 10 x (8N + 72K_i + 28C_i) + 8N (SURVEY.md 8(d) align); per step one "
                                         "conversion of `current` (6N + 64M: a uint16 frame); path_frac is per GPU",
                    "measured_in": "serial profiled pass of the same K steps (one stream, hipEvent pair per kernel stage)"}
        return dict(value=self.total * steps / dt, ms_per_step=dt / steps * 1e3, roofline=roofline, pipeline=pipe,
                    stage_ms_per_step={k: self.stage_ms[k] / max(steps, 1) for k in self.stage_ms},
                    accepted_by_closer_thresholds_rank0=accepted, max_translation_error_m_rank0=terr,
                    counters_mean={"M_current_frame": Mcur, "M_others": float(r["n_current"].mean()) if P else 0.0,
                                   "K_sum": float(b["Ks"].mean()) if P else 0.0, "C_sum": float(b["Cs"].mean()) if P else 0.0})

    def close(self):
        self.ctx.set_enqueued_callback(None)
        if getattr(self, "ticket", None) is not None:      # the look-ahead job of a step that will not come
            try:
                self.converter.computeExportEnd(self.ticket)
            except Exception:
                pass
            self.ticket = None
        if self.pipeline and self.use_dist:
            import torch
            for w_ in self.bw:                            # broadcasts of keyframes that will not be matched
                if w_ is not None:
                    w_.wait()
            torch.cuda.synchronize()
        self.others = None; self.current = None; self.replica = None; self.rep = None; self.conv_cloud = None
        self.ctx.close()
        if self.io is not None:
            self.io.close()


def launches_of(w):
    return max(w.stage_n["corr_linearize"], 1)


def closure_guesses(seeds, t_noise=0.01, q_noise=0.004):
    """initial guesses of a loop-closure candidate batch (pwn_tracker/pwn_closer.cpp:132-137: iT * other.T from the odometry): the true
    relative pose disturbed by a seeded error of <= 1 cm / ~0.5 deg per axis, with the z translation zeroed as
    PwnMatcherBase::matchClouds does (pwn_matcher_base.cpp:114).  Column-major float32 [n, 16]."""
    from g2o_frontend_amd import synth
    g = np.empty((len(seeds), 16), np.float32)
    for i, s in enumerate(seeds):
        u = synth._uniform(s, 7, 6)
        dv = np.concatenate([(2 * u[0:3] - 1) * t_noise, (2 * u[3:6] - 1) * q_noise])
        T = (synth.pair_pose(s) @ synth.v2t(dv)).astype(np.float32)
        T[2, 3] = 0.0; T[3] = (0, 0, 0, 1)
        g[i] = T.T.reshape(-1)
    return g


def run_extras_vga(w: BatchWorkload, args):
    """clouds are resident from the last step: the align-only and loop-closure lines of SURVEY.md §8(d)"""
    import ctypes as C
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import AlignResult, MatchResult
    out = {}
    P, steps, ctx = w.P, args.steps, w.ctx
    refs, curs, _ = w.align_prep
    p = w.aligner.params()
    L = ctx._L

    def stage_counts():
        return {k: ctx.stage_ms(k)[1] for k in ("project_cur", "project_ref", "corr_linearize")}

    # (1) align only, identity guess (warm cloud cache; the batch path takes the converter's own index images for the current cloud
    #     and for the first reference projection)
    res = (AlignResult * P)()
    ctx.check(L.pwn_hip_align_batch(ctx.h, C.byref(p), P, refs, curs, None, res))
    w.barrier(); a = time.perf_counter()
    for _ in range(steps):
        ctx.check(L.pwn_hip_align_batch(ctx.h, C.byref(p), P, refs, curs, None, res))
    w.barrier(); dt = time.perf_counter() - a
    ctx.set_profiling(True); ctx.check(L.pwn_hip_align_batch(ctx.h, C.byref(p), P, refs, curs, None, res)); sc = stage_counts(); ctx.set_profiling(False)
    nsub = max(1.0, sc["corr_linearize"] / max(w.n_it, 1))       # sub-batches the call was executed in (balanced over the streams by the library)
    r = np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=P)
    b = w.bytes_per_pair(r, sc["project_cur"] / nsub, sc["project_ref"] / nsub)
    out["align_only"] = {"alignments_per_s": P * steps / dt, "ms_per_step": dt / steps * 1e3, "guess": "identity",
                         "projections_per_pair": (sc["project_cur"] + sc["project_ref"]) / nsub,
                         "achieved_GBps": float(b["align"].sum()) * steps / dt / 1e9, "frac_of_peak": float(b["align"].sum()) * steps / dt / 1e9 / HBM_PEAK_GBS}
    # (2) the loop-closure call proper: pwn_hip_match_batch = align with per-pair non-identity guesses + matchClouds' depth-agreement
    #     score (pwn_matcher_base.cpp:114-119,153-182), acceptance of pwn_closer.cpp:138-141; every projection runs
    g = closure_guesses(w.seeds)
    scores = (MatchResult * P)()
    gp = g.ctypes.data_as(C.c_void_p)
    ctx.check(L.pwn_hip_match_batch(ctx.h, C.byref(p), P, refs, curs, gp, 50.0, res, scores))
    w.barrier(); a = time.perf_counter()
    for _ in range(steps):
        ctx.check(L.pwn_hip_match_batch(ctx.h, C.byref(p), P, refs, curs, gp, 50.0, res, scores))
    w.barrier(); dt = time.perf_counter() - a
    ctx.set_profiling(True); ctx.check(L.pwn_hip_match_batch(ctx.h, C.byref(p), P, refs, curs, gp, 50.0, res, scores)); sc = stage_counts(); ctx.set_profiling(False)
    nsub = max(1.0, sc["corr_linearize"] / max(w.n_it, 1))
    r = np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=P)
    b = w.bytes_per_pair(r, sc["project_cur"] / nsub, sc["project_ref"] / nsub)
    acc = api.PwnCloserAcceptance()
    accepted = sum(1 for m in scores if acc.accept(dict(image_nonZeros=m.image_non_zeros, image_outliers=m.image_outliers, image_inliers=m.image_inliers)))
    from g2o_frontend_amd import synth
    terr = max(float(np.abs(r["T"][i].reshape(4, 4).T[:3, 3] - synth.pair_pose(s)[:3, 3]).max()) for i, s in enumerate(w.seeds))
    out["closure_match_batch"] = {"alignments_per_s": P * steps / dt, "ms_per_step": dt / steps * 1e3,
                                  "guess": "true relative pose + seeded error <= 1 cm / 0.5 deg per axis, z translation zeroed (pwn_matcher_base.cpp:114)",
                                  "projections_per_pair": (sc["project_cur"] + sc["project_ref"]) / nsub, "scores": True,
                                  "accepted_by_closer_thresholds": accepted, "pairs": P, "max_translation_error_m": terr,
                                  "achieved_GBps": float(b["align"].sum()) * steps / dt / 1e9,
                                  "frac_of_peak": float(b["align"].sum()) * steps / dt / 1e9 / HBM_PEAK_GBS}
    # (3) PCIe-inclusive: the same step with the uint16 frames handed over from HOST memory (what a caller that holds cv::Mat-style host
    #     images pays): page-locked buffers of pwn_hip_host_alloc, and ordinary pageable arrays.  Never the headline value.
    hsteps = max(1, min(steps, 10))
    frames = [f[0] for f in w.frames_mm] + [f[1] for f in w.frames_mm]
    block = api.pinned_empty((len(frames),) + frames[0].shape, np.uint16)       # one block, like a grabber's ring: consecutive frames go in one transfer
    for i, f in enumerate(frames):
        block[i] = f
    hb = {}
    for name, host in (("pinned", [block[i] for i in range(len(frames))]), ("pageable", [np.ascontiguousarray(f) for f in frames])):
        prep = w.converter.batchHandles(w.refs + w.curs, host)

        def hstep():
            w.converter.computeBatch(w.refs + w.curs, host, raw_scale=0.001, prepared=prep)
            return w.aligner.alignBatch(w.refs, w.curs, raw=True, prepared=w.align_prep)
        hstep()
        w.barrier(); a = time.perf_counter()
        for _ in range(hsteps):
            r = hstep()
        w.barrier(); dt = time.perf_counter() - a
        hb[name] = {"alignments_per_s": P * hsteps / dt, "ms_per_step": dt / hsteps * 1e3}
        same = bool(np.array_equal(r["T"], w.last["res"]["T"]) and np.array_equal(r["chi2"], w.last["res"]["chi2"]))
        hb[name]["results_equal_to_resident_run"] = same
    # double-buffered upload (pwn_hip_copy_async): the frames of step k+1 travel while step k is being aligned
    dev = [ctx.upload(np.zeros(block.shape, np.uint16)) for _ in range(2)]
    prep = [w.converter.batchHandles(w.refs + w.curs, [d.frame(i) for i in range(len(frames))]) for d in dev]
    dev[0].copy_from_async(block)
    for timed in (False, True):
        w.barrier(); a = time.perf_counter()
        for it in range(hsteps if timed else 2):
            j = it % 2
            w.converter.computeBatch(w.refs + w.curs, None, raw_scale=0.001, prepared=prep[j])      # waits for the copies into dev[j]
            dev[1 - j].copy_from_async(block)
            r = w.aligner.alignBatch(w.refs, w.curs, raw=True, prepared=w.align_prep)
        w.barrier(); dt = time.perf_counter() - a
    hb["pinned_double_buffered"] = {"alignments_per_s": P * hsteps / dt, "ms_per_step": dt / hsteps * 1e3,
                                    "results_equal_to_resident_run": bool(np.array_equal(r["T"], w.last["res"]["T"]) and np.array_equal(r["chi2"], w.last["res"]["chi2"]))}
    for d in dev:
        d.free()
    api.pinned_free(block)
    out["host_frames"] = dict(hb, h2d_MB_per_step=2 * P * w.N * 2 / 1e6, steps=hsteps,
                              note="uint16 frames copied from host memory inside the step (2 x 614 KB per VGA pair) on the copy stream, one sub-batch ahead of the kernels; "
                                   "pinned = one pwn_hip_host_alloc block, pageable = separate numpy arrays; `value` is measured with the frames resident in HBM")
    return out


def run_tracker(device, frames_mm, poses, scale=1):
    """BASELINE configs[2]: PwnTracker::processFrame (pwn_tracker/pwn_tracker.cpp:106-215) over a 200-frame VGA stream, matcher scale 1;
    host float32 frames, uploaded inside the timed loop (the tracker's input is a host image)."""
    from g2o_frontend_amd import api, synth
    rows, cols, K = 480, 640, synth.K_VGA
    _, conv, alig = conf(rows, cols)
    ctx = api.Context(device, rows, cols, 2)
    converter, al = build_objects(ctx, rows, cols, K, conv, alig)
    alproj = api.PinholePointProjector(); alproj.setMinDistance(alig["min_distance"]); alproj.setMaxDistance(alig["max_distance"])
    al.setProjector(alproj)                          # the tracker re-configures the aligner's projector per frame (pwn_tracker.cpp:122-130)
    tracker = api.PwnTracker(al, converter); tracker.setScale(scale)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float32)
    I = np.eye(4, dtype=np.float32)
    frames = [ctx.DepthImage_convert_16UC1_to_32FC1(f) for f in frames_mm]
    tracker.processFrame(frames[0], I, Km); tracker.processFrame(frames[1], I, Km); tracker.init()      # warm-up
    t0 = time.perf_counter()
    for d in frames:
        tracker.processFrame(d, I, Km)
    dt = time.perf_counter() - t0
    true = np.linalg.inv(poses[0]) @ poses[len(frames) - 1]
    err = float(np.abs(tracker.globalT()[:3, 3] - true[:3, 3]).max())
    out = {"frames_per_s": len(frames) / dt, "frames": len(frames), "scale": scale, "ms_per_frame": dt / len(frames) * 1e3,
           "keyframes": tracker.numKeyframes(), "final_translation_error_m": err,
           "stream": "synth.trajectory_sweep(9): +-28 deg pan with sway, <= 2 cm and <= 1 deg per frame",
           "input": "host float32 frames (PCIe upload inside the timed loop)"}
    # the same stream with the next frame handed over one call ahead (a recorded / buffered stream: pwn_hip_convert_scaled_begin / _end):
    # makeCloud of frame k+1 runs next to the alignment of frame k; results are the same bits
    plainT, plainK = tracker.globalT().copy(), tracker.numKeyframes()
    tracker.init()
    tracker.prefetch(frames[0], I, Km); tracker.processFrame(frames[0], I, Km, nextDepthImage=frames[1]); tracker.init()      # warm-up: creates the helper context
    t0 = time.perf_counter()
    for k, d in enumerate(frames):
        tracker.processFrame(d, I, Km, nextDepthImage=frames[k + 1] if k + 1 < len(frames) else None)
    dt = time.perf_counter() - t0
    out["look_ahead"] = {"frames_per_s": len(frames) / dt, "ms_per_frame": dt / len(frames) * 1e3,
                         "bitwise_equal_to_plain": bool(np.array_equal(plainT.view(np.uint32), tracker.globalT().view(np.uint32)) and plainK == tracker.numKeyframes()),
                         "note": "frame k+1 converted by the library's helper thread while frame k is aligned"}
    ctx.close()
    return out


def run_tracker_cpp(frames_mm):
    """The same stream through the C++ host mirror (tools/pwn_hip_tracker_app: g2o_frontend_amd/host/pwn_hip.hpp over the C-ABI, 16-bit PGM files
    read before the clock starts, host float frames uploaded inside it): what the host side costs without the Python interpreter."""
    import re
    import subprocess
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from g2o_frontend_amd import build
    from run_cpp_tracker import CONF
    build.build_tools()
    exe = os.path.join(ROOT, "tools", "pwn_hip_tracker_app")
    with tempfile.TemporaryDirectory(prefix="pwn_trk_") as d:
        lst = []
        for k, f in enumerate(frames_mm):
            fn = os.path.join(d, f"d{k}.pgm")
            with open(fn, "wb") as fh:
                fh.write(b"P5\n%d %d\n65535\n" % (f.shape[1], f.shape[0])); fh.write(f.astype(">u2").tobytes())
            lst.append(f"{k * 0.033:.3f} {fn}")
        with open(os.path.join(d, "list.txt"), "w") as fh:
            fh.write("\n".join(lst) + "\n")
        out, tracks = {}, []
        for ahead in (0, 1):
            with open(os.path.join(d, "conf.txt"), "w") as fh:
                fh.write(CONF + f"lookAhead {ahead}\nwarmUp 1\n")
            prefix = os.path.join(d, f"run{ahead}")
            r = subprocess.run([exe, os.path.join(d, "conf.txt"), os.path.join(d, "list.txt"), prefix], capture_output=True, text=True, timeout=600)
            m = re.search(r"tracking: (\d+) frames, ([0-9.eE+-]+) ms per frame", r.stderr)
            if r.returncode != 0 or not m:
                raise RuntimeError("pwn_hip_tracker_app failed: " + r.stderr[-300:])
            ms = float(m.group(2))
            out["look_ahead" if ahead else "plain"] = {"frames_per_s": 1e3 / ms, "ms_per_frame": ms}
            tracks.append(open(prefix + "_track.txt", "rb").read())
        out["track_files_identical"] = tracks[0] == tracks[1]
        out["note"] = "tools/pwn_hip_tracker_app (C++ mirror), tracking loop with its track-file output; look_ahead = `lookAhead 1` (PwnTracker::prefetch)"
        return out


def run_single_pair_cpp():
    """configs[1] through the C++ host mirror (tools/pwn_hip_bench with one pair per step: convert 2 resident frames + align, 300 steps)"""
    import re
    import subprocess
    import tempfile
    from g2o_frontend_amd import build, synth
    build.build_tools()
    r, c, _ = synth.make_pair(0, 480, 640, synth.K_VGA)
    with tempfile.TemporaryDirectory(prefix="pwn_pair_") as d:
        names = []
        for tag, img in (("r", r), ("c", c)):
            fn = os.path.join(d, tag + ".pgm")
            with open(fn, "wb") as fh:
                fh.write(b"P5\n%d %d\n65535\n" % (img.shape[1], img.shape[0])); fh.write(img.astype(">u2").tobytes())
            names.append(fn)
        with open(os.path.join(d, "list.txt"), "w") as fh:
            fh.write("\n".join(names) + "\n")
        res = []
        for mode in ("0", "3"):      # 0: convert, then align (two calls); 3: one submission
            out = subprocess.run([os.path.join(ROOT, "tools", "pwn_hip_bench"), os.path.join(d, "list.txt"), "1", "300", "10", "0", mode],
                                 capture_output=True, text=True, timeout=300)
            m = re.search(r"ms_per_step ([0-9.eE+-]+)", out.stdout)
            if out.returncode != 0 or not m:
                raise RuntimeError("pwn_hip_bench failed: " + (out.stderr or out.stdout)[-300:])
            res.append(float(m.group(1)))
        return res


def run_tracker_replicas(device, frames_mm, replicas=4, scale=1):
    """the tracker is serial across frames -- more streams, not more GPUs per stream.  `replicas` independent trackers
    (one context and one host thread each, the same 200 frames) on ONE GPU: a single VGA pair fills 150 of the 256 CUs for a few
    microseconds at a time, so the launches of different streams interleave."""
    import threading
    from g2o_frontend_amd import api, synth
    rows, cols, K = 480, 640, synth.K_VGA
    _, conv, alig = conf(rows, cols)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float32)
    I = np.eye(4, dtype=np.float32)
    ctx0 = api.Context(device, rows, cols, 2)
    frames = [ctx0.DepthImage_convert_16UC1_to_32FC1(f) for f in frames_mm]
    ctx0.close()
    gate = threading.Barrier(replicas + 1)
    finals, errors = [None] * replicas, []

    def stream(k):
        try:
            ctx = api.Context(device, rows, cols, 2)
            converter, al = build_objects(ctx, rows, cols, K, conv, alig)
            alproj = api.PinholePointProjector(); alproj.setMinDistance(alig["min_distance"]); alproj.setMaxDistance(alig["max_distance"])
            al.setProjector(alproj)
            tracker = api.PwnTracker(al, converter); tracker.setScale(scale)
            tracker.processFrame(frames[0], I, Km); tracker.processFrame(frames[1], I, Km); tracker.init()
            gate.wait(); gate.wait()
            for d in frames:
                tracker.processFrame(d, I, Km)
            finals[k] = tracker.globalT().copy()
            gate.wait()
            ctx.close()
        except Exception as e:      # a failing stream must not leave the others waiting at the gate
            errors.append(repr(e)); gate.abort()

    threads = [threading.Thread(target=stream, args=(k,)) for k in range(replicas)]
    for t in threads:
        t.start()
    try:
        gate.wait(); t0 = time.perf_counter(); gate.wait()
        gate.wait(); dt = time.perf_counter() - t0
    except threading.BrokenBarrierError:
        dt = None
    for t in threads:
        t.join()
    if dt is None or errors:
        return {"replicas": replicas, "error": "; ".join(errors) or "barrier broken"}
    return {"replicas": replicas, "frames_per_s_total": replicas * len(frames) / dt, "frames_per_stream": len(frames), "scale": scale,
            "ms_per_frame_per_stream": dt / len(frames) * 1e3,
            "streams_bitwise_equal": bool(all(np.array_equal(finals[0], f) for f in finals[1:])),
            "note": "independent tracker streams on one GPU, one context + host thread each (Python threads; ctypes releases the GIL during the calls)"}


def chi2_match(traces, res, w=None):
    """The chi2 parity gate that travels with the throughput number.  Teacher-forced (the gate, bar 1e-5): every iteration
    of the CPU oracle's trace re-run on the GPU from the oracle's own iterate -- the same inputs on both sides, so K_i, C_i, inliers_i
    must be equal and chi2_i within 1e-5 of the oracle's fp64-accumulated sum.  Free-running (reported): this run's headline results
    against the oracle's own 10-iteration trace; the iterates then differ in their last bits (summation order of H, b), a projected point
    can cross a pixel border and one correspondence entering or leaving moves chi2 by ~1/C."""
    worst64 = worst32 = worstT = 0.0
    for t in traces:
        g = res[t["seed"]]
        n = int(g["iterations"])
        for k in range(min(n, len(t["chi2_fp64"]))):
            worst64 = max(worst64, abs(float(g["chi2"][k]) - t["chi2_fp64"][k]) / max(t["chi2_fp64"][k], 1e-30))
            worst32 = max(worst32, abs(float(g["chi2"][k]) - t["chi2_fp32_serial"][k]) / max(t["chi2_fp32_serial"][k], 1e-30))
        worstT = max(worstT, float(np.abs(g["T"].reshape(4, 4).T - np.asarray(t["T"])).max()))
    out = {"pairs": len(traces), "bar": 1e-5, "bar_applies_to": "teacher-forced comparison (max_rel_diff): same iterate on both sides",
           "free_running_bar": FREE_RUNNING_CHI2_BAR,
           "free_running_note": "seed-dependent: one correspondence entering or leaving the set moves chi2 by its own term (~1/C = 5e-6 of chi2 at VGA, "
                                "20-40 x that for a term at the finder's thresholds); measured worst over 16 VGA seeds 1.9e-4 (tests/test_gpu_parity.py::test_free_running_chi2_many_seeds)",
           "free_running_max_rel_diff_vs_fp64_accumulated_oracle": worst64, "free_running_ok": bool(worst64 <= FREE_RUNNING_CHI2_BAR),
           "free_running_max_rel_diff_vs_reference_fp32_serial_sums": worst32, "free_running_max_abs_pose_diff": worstT,
           "note": "fp32-serial = the reference's own summation order: the distance between two orders of the same fp32 terms (tests allow 1e-4 / 5e-3)"}
    if w is not None and traces and "T_before" in traces[0]:
        al = w.aligner
        outer, guess = al._outerIterations, al._initialGuess.copy()
        import zlib
        worst_tf, counters_equal, index_equal, n_it = 0.0, True, True, 0
        al.setOuterIterations(1)
        try:
            for t in traces:
                i = w.seeds.index(t["seed"])
                al.setReferenceCloud(w.refs[i]); al.setCurrentCloud(w.curs[i])
                for k, Tb in enumerate(t["T_before"]):
                    al.setInitialGuess(np.asarray(Tb, np.float32))
                    last = k == len(t["T_before"]) - 1 and "index_crc" in t
                    g = al.align(images=last)
                    worst_tf = max(worst_tf, abs(float(g["chi2"][0]) - t["chi2_fp64"][k]) / max(t["chi2_fp64"][k], 1e-30))
                    counters_equal = counters_equal and [int(g["K"][0]), int(g["C"][0]), int(g["iter_inliers"][0])] == t["counters"][k]
                    if last:
                        f = al.correspondenceFinder()
                        index_equal = index_equal and [zlib.crc32(f.referenceIndexImage().tobytes()), zlib.crc32(f.currentIndexImage().tobytes())] == t["index_crc"]
                    n_it += 1
        finally:
            al.setOuterIterations(outer); al.setInitialGuess(guess)
        out.update(mode="teacher-forced: each oracle iteration re-run on the GPU from the oracle's iterate (same inputs both sides)",
                   max_rel_diff=worst_tf, iterations_checked=n_it, counters_equal=bool(counters_equal),
                   projector_index_images_bit_exact=bool(index_equal), ok=bool(worst_tf <= 1e-5 and counters_equal and index_equal),
                   canonical_choices="single-thread semantics of the finder / linearizer; eigensolver trig by the shared double-precision algorithm (DESIGN.md section 2)")
    else:
        out.update(mode="free-running only", max_rel_diff=worst64, ok=bool(worst64 <= FREE_RUNNING_CHI2_BAR))
    return out


# ------------------------------------------------------------------------------------------------ record digests (determinism gate)
RECORDS_CRC_FILE = os.path.join(ROOT, "profiles", "records_crc.json")


CRC_DIR = os.path.dirname(RECORDS_CRC_FILE)


def records_crc_file(mode="pairs", omega_storage="sym6"):
    """one digest file per (workload, omega storage): the bench default (pairs, sym6) keeps the historical name"""
    if mode == "pairs" and omega_storage == "sym6":
        return os.path.join(CRC_DIR, "records_crc.json")
    return os.path.join(CRC_DIR, "records_crc_%s_%s.json" % (mode, omega_storage))


def records_crc(allrec):
    """CRC32 of every assembled 256-byte result record (shard.py: pose, final values, per-iteration traces, counts, pair id), in global pair order"""
    import zlib
    a = np.ascontiguousarray(allrec, np.float32)
    return [int(zlib.crc32(a[i].tobytes())) for i in range(a.shape[0])]


def kernel_source_digest():
    """identifies the kernels a records_crc.json belongs to: a change of summation order changes the last bits of H, b and so the records"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "g2o_frontend_amd", "csrc")
    for f in sorted(os.listdir(d)):
        h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def check_records_crc(allrec, rows, cols, write=False, omega_storage="exact9", mode="pairs"):
    crc = records_crc(allrec)
    src = kernel_source_digest()
    fn = records_crc_file(mode, omega_storage)
    rel = os.path.relpath(fn, ROOT)
    if write:
        with open(fn, "w") as f:
            json.dump({"made_by": "bench.py --gpus 1 --mode %s --omega-storage %s --total-pairs %d --write-records-crc (one MI355X)" % (mode, omega_storage, len(crc)),
                       "rows": rows, "cols": cols, "mode": mode,
                       "omega_storage": omega_storage, "kernel_source_digest": src, "pairs": len(crc), "crc32": crc}, f)
    if not os.path.exists(fn):
        return {"checked": 0, "note": "no " + rel}
    try:
        g = json.load(open(fn))
    except Exception as e:
        return {"checked": 0, "note": "unreadable: %r" % (e,)}
    if (g.get("rows"), g.get("cols")) != (rows, cols):
        return {"checked": 0, "note": "file is for another frame size"}
    if g.get("omega_storage", "exact9") != omega_storage:
        return {"checked": 0, "note": "file is for omega_storage = %s" % g.get("omega_storage", "exact9")}
    n = min(len(crc), g["pairs"])
    bad = [i for i in range(n) if crc[i] != g["crc32"][i]]
    return {"checked": n, "equal": not bad, "first_mismatch": bad[0] if bad else None, "mismatches": len(bad),
            "file_is_for_these_kernels": g.get("kernel_source_digest") == src, "file": rel,
            "note": "records of pair p are the same bits whatever GPU / rank / sub-batch aligned it; a mismatch with a stale file (other kernel sources) means nothing"}


DUMP_MAX_BYTES = 64 << 20


def timed_outputs(last, total, seeds):
    """{name: float32 / float64 array} of what the last timed step returned: every field of the rank's result array except the host timing
    (in partition mode also the four depth-agreement scores per pair), the rank's global pair ids, and the records of every pair of the job
    in global pair order"""
    from g2o_frontend_amd import shard
    res, sc = last["res"] if isinstance(last["res"], tuple) else (last["res"], None)
    out = {"pair_ids": np.asarray(seeds, np.float64)}
    for name in (res.dtype.names if res is not None else ()):      # a rank without pairs of its own has no result array
        if name == "total_time_ms":
            continue
        a = res[name]
        out[name] = a.astype(np.float64) if a.dtype.kind in "iu" else a.astype(np.float32)
    if sc is not None:
        out["scores"] = np.asarray([(m.image_non_zeros, m.image_outliers, m.image_inliers, m.image_reprojection_distance) for m in sc], np.float64)
    out["records"] = np.ascontiguousarray(shard.assemble(last["gathered"], total), np.float32)
    return out


def dump_outputs(d, arrays, max_bytes=DUMP_MAX_BYTES):
    """DIR/<name>.npy per array; above max_bytes in all, every array keeps the same fraction of its rows, chosen by a fixed seed"""
    os.makedirs(d, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > max_bytes and a.ndim and a.shape[0] > 1:
            keep = max(1, int(a.shape[0] * max_bytes / total))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(d, name + ".npy"), a)
    return sorted(arrays)


# ------------------------------------------------------------------------------------------------ CPU dry run of the N-rank plumbing
def dry_run_cpu(args, rank, world):
    """launcher -> ranks -> shard -> records (the real pwn_hip_align_result layout) -> all-gather (gloo) -> assemble, no GPU"""
    import torch
    import torch.distributed as dist
    from g2o_frontend_amd import shard
    from g2o_frontend_amd.api import ALIGN_RESULT_DTYPE
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    P = args.pairs
    total = args.total_pairs if args.total_pairs > 0 else world * P
    seeds = list(shard.shard_range(total, rank, world))
    P = len(seeds); Pmax = (total + world - 1) // world
    res = np.zeros(P, ALIGN_RESULT_DTYPE)
    for i, s in enumerate(seeds):      # what pwn_hip_align_batch would have filled in for pair s
        T = np.eye(4, dtype=np.float32); T[:3, 3] = (s, 2 * s, -s)
        res["T"][i] = T.T.reshape(-1); res["error"][i] = 0.5 * s; res["inliers"][i] = 1000 + s; res["iterations"][i] = 10
    packed = shard.pack_results_raw(res, seeds)
    flat_ok = None
    if args.mode == "partition":
        # the byte path of --mode partition: a flat `current` cloud (here: a seeded byte pattern of a flat cloud's size) broadcast from rank 0,
        # every rank checks what arrived; the records carry the four score words of PWN_HIP_MATCH_RECORD_FLOATS behind the alignment record
        nbytes = 256 + 3 * ((P * 4 + 255) // 256 * 256)
        pattern = (np.arange(nbytes, dtype=np.uint64) * 2654435761 % 251).astype(np.uint8)
        flat = torch.from_numpy(pattern.copy() if rank == 0 else np.zeros(nbytes, np.uint8))
        if world > 1:
            dist.broadcast(flat, src=0)
        pipe = simulate_partition_pipeline_cpu(rank, world, 11, dist)      # the pipelined step's bookkeeping with flat clouds of varying size
        ok = torch.tensor([1.0 if (np.array_equal(flat.numpy(), pattern) and pipe) else 0.0], dtype=torch.float64)
        if world > 1:
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        flat_ok = bool(ok.item() == 1.0)
        packed = np.concatenate([packed, np.zeros((P, 8), np.float32)], axis=1)
        for i, sd in enumerate(seeds):
            packed[i, 64:68] = (3000 + sd, sd % 7, 2900 + sd, 0.25 * sd)
    rec = torch.from_numpy(packed)
    g = shard.gather_records(rec, world, Pmax)
    t = torch.tensor([float(rank)], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.barrier()
    if rank == 0:
        allrec = shard.assemble(g.numpy(), total)
        ok = all(allrec[p, 12] == p and allrec[p, 13] == 2 * p and allrec[p, 14] == -p and allrec[p, 17] == 1000 + p and allrec[p, 19] == p
                 for p in range(total))
        if args.mode == "partition":
            ok = ok and allrec.shape[1] == 72 and all(allrec[p, 64] == 3000 + p and allrec[p, 66] == 2900 + p and allrec[p, 67] == 0.25 * p for p in range(total))
        print(json.dumps({"dry_run": True, "n_gpus": world, "mode": args.mode, "flat_cloud_broadcast_ok": flat_ok, "records": int(allrec.shape[0]), "records_ok": bool(ok), "max_rank_seen": int(t.item()),
                          "pairs_per_gpu": P, "scaling": "strong" if args.total_pairs > 0 else "weak", "total_pairs": total,
                          "records_crc": records_crc(allrec)[:4], "records_crc_all": int(zlib.crc32(np.asarray(records_crc(allrec), np.uint32).tobytes())),
                          "rank0_cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None}))
    if world > 1:
        dist.destroy_process_group()


def host_cpu_info():
    """what the `cores` of cpu_baseline are: logical cpus this process may use, physical cores among them, SMT, the cgroup's cpu quota"""
    out = {}
    try:
        cpus = sorted(os.sched_getaffinity(0))
        out["logical_cpus"] = len(cpus)
        cores = set()
        for c in cpus:
            try:
                with open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list") as f:
                    cores.add(f.read().strip())
            except Exception:
                cores.add(str(c))
        out["physical_cores"] = len(cores)
        out["smt"] = len(cores) < len(cpus)
    except Exception:
        pass
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()
            quota = None if q == "max" else float(q) / float(per)
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            quota = None if q < 0 else q / per
        except Exception:
            quota = None
    out["cgroup_cpu_quota"] = quota
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    out["cpu_model"] = line.split(":", 1)[1].strip(); break
    except Exception:
        pass
    return out


def multi_gpu_diagnostics(w, args, rank, world, dt_rank, dt_serial, pinned, n_collective=20):
    """Per-rank evidence for a scaling run (the builder cannot iterate on 8 GPUs, the line has to explain itself): every rank's own ms per step of
    the timed region and of the serial profiled pass, its per-stage device times, the cores it was pinned to, and the collectives timed alone."""
    import torch
    import torch.distributed as dist
    keys = sorted(w.stage_ms)
    mine = [dt_rank / max(args.steps, 1) * 1e3, (dt_serial or 0.0) / max(args.steps, 1) * 1e3,
            float(len(pinned)) if pinned else 0.0, float(pinned[0]) if pinned else -1.0, float(pinned[-1]) if pinned else -1.0]
    mine += [w.stage_ms[k] / max(args.steps, 1) for k in keys]
    t = torch.tensor(mine, dtype=torch.float64, device="cuda")
    allt = torch.empty((world, len(mine)), dtype=torch.float64, device="cuda")
    from g2o_frontend_amd import shard
    shard.all_gather_into(allt, t)
    coll = w.time_collectives(n_collective)
    a = allt.cpu().numpy()
    return {"per_rank_ms_per_step": [float(x) for x in a[:, 0]], "per_rank_serial_pass_ms_per_step": [float(x) for x in a[:, 1]],
            "rank_cpus": [{"count": int(r[2]), "first": int(r[3]), "last": int(r[4])} for r in a],
            "per_rank_stage_ms_per_step": {k: [float(x) for x in a[:, 5 + i]] for i, k in enumerate(keys)},
            "collectives_alone": dict(coll, steps=n_collective, note="no compute between the collectives; ms per call, this rank's clock after a device sync")}


_T0 = time.time()


def _progress(rank, world, msg):
    """one stderr line per phase and rank in multi-rank runs: the 8-GPU run cannot be repeated, so if a rank stalls the log says where"""
    if world > 1:
        print(f"[bench rank {rank}/{world} +{time.time() - _T0:6.1f}s] {msg}", file=sys.stderr, flush=True)


# ------------------------------------------------------------------------------------------------ main
def main():
    args = parse()
    if args.cpu_baseline_only:
        return cpu_baseline_child(args)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N`: become the launcher; the ranks are children started before any GPU call (this process makes none)
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", 0)); world = int(os.environ.get("WORLD_SIZE", 1)); local = int(os.environ.get("LOCAL_RANK", 0))
    if args.one_device:
        local_cpu, local = local, 0           # the rank's block of host cores still follows LOCAL_RANK; its GPU is device 0
    else:
        local_cpu = local
    pinned = pin_rank(local_cpu, int(os.environ.get("LOCAL_WORLD_SIZE", world))) if world > 1 else None      # before the render pool and before any GPU call
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a number for a different GPU count", file=sys.stderr)
        sys.exit(2)
    if args.dry_run_cpu:
        return dry_run_cpu(args, rank, world)
    if world > 1 or os.environ.get("PWN_BENCH_FORCE_DIST") == "1":
        # A rank of a multi-GPU run has more streams than the library's four: the collectives' stream, the side streams the broadcast, the all-gather and
        # the import are ordered on, the look-ahead helper's.  The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues
        # (default 4), and two of the library's compute streams that land on one queue run one after the other.  Measured at world size 1 through RCCL
        # (docs/experiments.md, round 6): partition step 6.54-6.57 ms with 4 queues, 6.46-6.49 with 8 (plain: 6.38); pairs step unchanged.  Read by the
        # runtime when it initialises, i.e. at the first HIP call of this process -- nothing has made one yet.
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    rows, cols, P = args.rows, args.cols, args.pairs
    K, conv, alig = conf(rows, cols)
    partition = args.mode == "partition"
    full = args.full
    extras_on = full and rank == 0 and world == 1 and not args.no_extras and not partition      # the extra lines are single-GPU measurements of the headline workload

    # CPU baseline first (rank 0 at N = 1 only: the other ranks of a multi-GPU run would wait for it), in a child process started
    # before anything touches the GPU: the process that drives the GPU never loads the oracle library
    cpu = None
    traces = None
    if full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--rows", str(rows), "--cols", str(cols),
                              "--cpu-seconds", str(args.cpu_seconds)], capture_output=True, text=True, timeout=900)
        try:
            cpu = json.loads(out.stdout.strip().splitlines()[-1])
            traces = cpu.pop("chi2_traces", None)
            cpu.update(host_cpu_info())
            if partition:
                cpu["note"] = ("the sample is the pairs workload (convert 2 frames + align per item); an item of --mode partition is ONE alignment from an odometry "
                               "guess + the depth-agreement score against a cached cloud: compare with align_only_single_thread_value")
        except Exception:
            cpu = {"error": (out.stderr or out.stdout)[-300:]}

    # synthetic inputs of this rank's shard (and of the extra lines), rendered on the CPU before the GPU is initialised
    from g2o_frontend_amd import shard, synth
    total = args.total_pairs if args.total_pairs > 0 else world * P      # strong scaling: the same pair list whatever N is; weak: --pairs per rank
    if total < world:
        print("bench.py: fewer pairs than ranks", file=sys.stderr); sys.exit(2)
    seeds = list(shard.shard_range(total, rank, world))                  # contiguous shard of the global pair list
    P = len(seeds)
    n5 = 0; poses = None
    if partition:
        jobs = partition_jobs(seeds, rows, cols, K) + [("frame", PARTITION_SCENE, np.eye(4).tolist(), rows, cols, K, 0)]      # the shard's keyframes + `current`
    else:
        jobs = [("pair", s, rows, cols, K) for s in seeds]
    if extras_on and not args.no_config5 and (rows, cols) == (480, 640):
        n5 = 32
        jobs += [("pair", s, 960, 1280, synth.K_1280) for s in range(n5)]
    if extras_on and not args.no_tracker and (rows, cols) == (480, 640):
        poses = synth.trajectory_sweep(9, args.tracker_frames)
        jobs += [("frame", 9, poses[k].tolist(), 480, 640, synth.K_VGA, k) for k in range(args.tracker_frames)]
    # a pinned rank owns its cores: the pool takes all of them; unpinned ranks share the box (cores // world each)
    _progress(rank, world, f"pinned to {len(pinned) if pinned else 0} cpus; rendering {len(jobs)} jobs")
    rendered = render_all(jobs, 1 if pinned else world, args.render_workers)
    _progress(rank, world, "frames rendered; initialising the GPU and the process group")
    nmain = P + 1 if partition else P
    frames_mm = rendered[:nmain]; frames5 = rendered[nmain:nmain + n5]; frames_trk = rendered[nmain + n5:]

    import torch
    import torch.distributed as dist
    torch.cuda.set_device(local)
    use_dist = world > 1 or os.environ.get("PWN_BENCH_FORCE_DIST") == "1"      # FORCE_DIST: exercise the RCCL path at world size 1
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        # RCCL prints a version banner on stdout when the communicator is created; keep stdout for the one JSON line
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            if args.one_device:
                dist.init_process_group("gloo", rank=rank, world_size=world)
            else:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
            dist.barrier()
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)
    n_seen = dist.get_world_size() if use_dist else 1                            # the ranks the process group actually holds
    _progress(rank, world, f"process group of {n_seen} up; building the workload ({P} items)")

    if partition:
        w = PartitionWorkload(args, local, rows, cols, seeds, frames_mm[:P], frames_mm[P], use_dist, world, rank, total)
    else:
        w = BatchWorkload(args, local, rows, cols, P, frames_mm, seeds, use_dist, world)
        w.total = total; w.Pmax = (total + world - 1) // world
    profile = full and not args.no_profile
    _progress(rank, world, "workload resident; warm-up + timed region" + (" + serial profiled pass" if profile else ""))
    dt_rank, dt_serial = w.run(args.steps, args.warmup, profile=profile)
    _progress(rank, world, f"timed region {dt_rank / max(args.steps, 1) * 1e3:.3f} ms per step on this rank")
    dt = dt_rank
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    rep = w.report(args.steps, dt, dt_serial, world)
    # what a sub-linear scaling curve would have to be explained with: every rank's own step time, the collectives alone, the cores each rank ran on
    multi = multi_gpu_diagnostics(w, args, rank, world, dt_rank, dt_serial, pinned) if (use_dist and full) else None
    gather_info = None
    if rank == 0 and (full or args.write_records_crc):      # writing the digests is asked for by name: it does not need --full
        allrec = shard.assemble(w.last["gathered"].cpu().numpy(), total)          # every pair of every rank arrived exactly once
        assert allrec.shape[0] == total
        if partition:
            res, sc = w.last["res"]
            mine = shard.pack_results_raw(res, seeds)
            mine = np.concatenate([mine, np.zeros((len(seeds), 8), np.float32)], axis=1)
            for i, m in enumerate(sc):
                mine[i, 64:68] = (m.image_non_zeros, m.image_outliers, m.image_inliers, m.image_reprojection_distance)
        else:
            mine = shard.pack_results_raw(w.last["res"], seeds)                    # this rank's own records as they left the C-ABI
        gather_info = {"backend": ("gloo on device tensors (--one-device rehearsal)" if args.one_device else "nccl (RCCL), all_gather_into_tensor on device tensors") if use_dist
                       else "none (one rank: the local records)",
                       "forced": bool(use_dist and world == 1), "world": n_seen, "records": int(allrec.shape[0]), "record_bytes": int(4 * allrec.shape[1]),
                       "records_equal_local": bool(np.array_equal(allrec[np.asarray(seeds)].view(np.uint32), mine.view(np.uint32)))}
        # determinism gate of the multi-GPU leg: a pair's record does not depend on which GPU aligned it, in which sub-batch or next to which
        # other pairs (tests/test_gpu_properties.py) -- nor, in partition mode, on whether the `current` cloud is the converted original or a replica
        # that travelled through export / broadcast / import -- so the records any N assembles must equal, bit for bit, those of the one-GPU run
        gather_info["records_vs_single_gpu_run"] = check_records_crc(allrec, rows, cols, write=args.write_records_crc and world == 1 and not use_dist,
                                                                     omega_storage=args.omega_storage, mode=args.mode)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, timed_outputs(w.timed_last, total, seeds))

    extra = {}
    if full and not args.no_latency and rank == 0 and world == 1 and not partition:
        lat = []
        for _ in range(5):
            torch.cuda.synchronize(); a = time.perf_counter()
            w.converter.computeBatch([w.refs[0], w.curs[0]], [w.ref_dev[0], w.cur_dev[0]], raw_scale=0.001)
            w.aligner.alignBatch([w.refs[0]], [w.curs[0]])
            lat.append((time.perf_counter() - a) * 1e3)
        extra["single_pair_latency_ms"] = float(np.median(lat))
        # the same pair as ONE submission (pwn_hip_convert_align_batch_u16 with n = 1: one host wait instead of two; same bits)
        lat1 = []
        h1 = w.aligner.convertAlignHandles([w.refs[0]], [w.curs[0]], [w.ref_dev[0]], [w.cur_dev[0]], converter=w.converter)
        for _ in range(7):
            torch.cuda.synchronize(); a = time.perf_counter()
            w.aligner.convertAlignBatch(w.converter, None, None, None, None, raw_scale=0.001, prepared=h1)
            lat1.append((time.perf_counter() - a) * 1e3)
        extra["single_pair_latency_ms_one_submission"] = float(np.median(lat1[2:]))
        w.step()                                                                   # clouds of all pairs resident again
    if rank == 0 and traces and not partition:
        extra["chi2_match"] = chi2_match(traces, w.last["res"], w)
    hbm_read = hbm_copy = None
    if full and rank == 0 and world == 1:      # (at N > 1 the other ranks would wait in the final barrier meanwhile)
        try:      # the bandwidth this box actually delivers, next to the 8 TB/s spec figure (float4 streaming read / copy of 2 GiB)
            hbm_read, hbm_copy = w.ctx.measure_hbm(1 << 31)
        except Exception:
            hbm_read = hbm_copy = None
    if extras_on:
        try:
            extra.update(run_extras_vga(w, args))
        except Exception as e:
            extra["extras_error"] = repr(e)[:300]
    w.close()
    if extras_on and args.omega_storage == "sym6":
        # the library's default storage (exact9: every converter output bit-identical to the CPU path) on the same pairs, so that the line
        # carries both modes (the headline runs sym6: lower triangle of Omega_p mirrored, chi2 / H / b within 1e-5)
        try:
            a9 = argparse.Namespace(**vars(args)); a9.omega_storage = "exact9"
            w9 = BatchWorkload(a9, local, rows, cols, P, frames_mm, seeds, False, 1)
            s9 = max(2, min(args.steps, 5))
            d9, _ = w9.run(s9, 1, profile=False)
            r9 = w9.report(s9, d9, None, 1)
            allrec9 = shard.pack_results_raw(w9.last["res"], seeds)
            extra["omega_exact9"] = {"alignments_per_s": r9["value"], "ms_per_step": r9["ms_per_step"], "steps": s9, "path_frac": r9["roofline"]["path_frac"],
                                     "algorithmic_bytes_per_pair": r9["path_roofline"]["algorithmic_bytes_per_pair"],
                                     "note": "same step with omega_storage = exact9 (36-byte point information matrices, the library default); the byte count "
                                             "keeps SURVEY.md 8(d)'s 24-byte figure",
                                     "records_vs_single_gpu_run": check_records_crc(allrec9, rows, cols, omega_storage="exact9", mode="pairs")}
            w9.close()
        except Exception as e:
            extra["omega_exact9_error"] = repr(e)[:300]
    if extras_on and n5:
        try:
            a5 = argparse.Namespace(**vars(args)); a5.sub_frames = min(args.sub_frames, 2 * n5); a5.sub_pairs = min(args.sub_pairs, n5)
            w5 = BatchWorkload(a5, local, 960, 1280, n5, frames5, list(range(n5)), False, 1)
            s5 = max(2, min(args.steps, 5))
            d5, d5s = w5.run(s5, 1, profile=True)
            r5 = w5.report(s5, d5, d5s, 1)
            extra["config5_1280x960"] = {"alignments_per_s": r5["value"], "ms_per_step": r5["ms_per_step"], "pairs_per_gpu": n5, "steps": s5,
                                         "workload": "BASELINE configs[4] shard: 32 pairs of 1280x960 (256 over 8 GPUs), convert 2 frames + align",
                                         "roofline": r5["roofline"], "path_roofline": r5["path_roofline"], "stage_ms_per_step": r5["stage_ms_per_step"]}
            w5.close()
        except Exception as e:
            extra["config5_error"] = repr(e)[:300]
    if extras_on and poses is not None:
        try:
            extra["tracker_config2"] = run_tracker(local, frames_trk, poses)
            extra["tracker_config2"]["replicas_on_one_gpu"] = run_tracker_replicas(local, frames_trk, replicas=4)
            try:
                extra["single_pair_latency_ms_cpp_mirror"], extra["single_pair_latency_ms_cpp_mirror_one_submission"] = run_single_pair_cpp()
            except Exception as e:
                extra["single_pair_cpp_error"] = repr(e)[:300]
            try:
                extra["tracker_config2"]["cpp_mirror"] = run_tracker_cpp(frames_trk)
            except Exception as e:
                extra["tracker_config2"]["cpp_mirror"] = {"error": repr(e)[:300]}
        except Exception as e:
            extra["tracker_error"] = repr(e)[:300]

    if full and rank == 0 and rep.get("path_roofline"):
        # the latency configurations against the same peak (BASELINE configs[1], [2]): algorithmic bytes of ONE pair / ONE tracked frame over the
        # measured latency.  One pair is a chain of ~35 dependent launches of 150-600 workgroups each: it cannot fill the memory system, and the
        # fraction says by how much (missing #5)
        pr_ = rep["path_roofline"]; pair_bytes = pr_["algorithmic_bytes_per_pair"]
        align_bytes_pair = pair_bytes - pr_["convert_bytes_per_pair"]
        for key in ("single_pair_latency_ms", "single_pair_latency_ms_one_submission", "single_pair_latency_ms_cpp_mirror", "single_pair_latency_ms_cpp_mirror_one_submission"):
            if isinstance(extra.get(key), (int, float)) and extra[key] > 0:
                extra[key.replace("latency_ms", "roofline_frac")] = pair_bytes / (extra[key] * 1e-3) / 1e9 / HBM_PEAK_GBS
        trk = extra.get("tracker_config2")
        if isinstance(trk, dict) and trk.get("ms_per_frame"):
            # a tracked frame: one float32 frame converted (2N more input than a u16 frame) + one alignment against the key cloud
            frame_bytes = pr_["convert_bytes_per_pair"] / 2 + 2.0 * rows * cols + align_bytes_pair
            trk["algorithmic_bytes_per_frame"] = frame_bytes
            trk["roofline_frac"] = frame_bytes / (trk["ms_per_frame"] * 1e-3) / 1e9 / HBM_PEAK_GBS
            cm = trk.get("cpp_mirror") if isinstance(trk.get("cpp_mirror"), dict) else {}
            for q in (trk.get("look_ahead"), cm.get("plain"), cm.get("look_ahead")):
                if isinstance(q, dict) and q.get("ms_per_frame"):
                    q["roofline_frac"] = frame_bytes / (q["ms_per_frame"] * 1e-3) / 1e9 / HBM_PEAK_GBS
            extra["tracker_roofline_frac"] = trk["roofline_frac"]
            trk["roofline_note"] = ("align term: the headline batch's mean per-pair counters (identity guess, 9 of 11 projections); the tracker's guesses are not the "
                                    "identity (11 of 11), so the fraction is a lower bound by ~2 projections' bytes (~3 %)")
        if "single_pair_roofline_frac" in extra:
            extra["single_pair_roofline_frac_note"] = "algorithmic bytes of one pair (path_roofline.algorithmic_bytes_per_pair) / single_pair_latency_ms / 8 TB/s"
    if rank == 0:
        if partition:
            workload = (f"PwnCloser::processPartition: one {cols}x{rows} `current` frame (converted per step on rank 0, its cloud broadcast to every GPU) matched "
                        f"against {P} cached keyframe clouds per GPU (matchClouds: Aligner::align {alig['outer_iterations']}x{alig['inner_iterations']} GN iterations "
                        f"from an odometry guess + depth-agreement score); SURVEY.md 8(e) partitioning")
            parallelism = f"cached clouds sharded over {n_seen} GPU(s); RCCL broadcast of the `current` cloud (~17 MB) + all-gather of 288-byte records"
        else:
            workload = (f"loop-closure batch: {P} independent {cols}x{rows} depth pairs per GPU "
                        f"(u16 mm frames resident in HBM; per pair: convert 2 frames + Aligner::align, "
                        f"{alig['outer_iterations']}x{alig['inner_iterations']} GN iterations); BASELINE configs[3] shard")
            parallelism = f"independent pairs sharded over {n_seen} GPU(s), RCCL all-gather of result records only"
        out = {
            "metric": "depth-pair alignments/sec (640x480, 10 GN iters)", "value": rep["value"], "unit": "alignments/s",
            "n_gpus": n_seen, "steps": args.steps, "warmup": args.warmup, "ms_per_step": rep["ms_per_step"],
            "higher_is_better": True, "scaling": "strong" if args.total_pairs > 0 else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": workload, "mode": args.mode,
                       "pairs_per_gpu": P, "total_pairs": total, "rows": rows, "cols": cols, "sub_frames": args.sub_frames, "sub_pairs": args.sub_pairs,
                       "streams": args.streams, "omega_storage": args.omega_storage, "step_mode": args.step_mode if not partition else None,
                       "parallelism": parallelism,
                       "rehearsal": (f"{n_seen} rank processes on ONE device, collectives through gloo: a correctness rehearsal of the multi-rank step, "
                                     f"not a scaling measurement") if args.one_device else None,
                       "cpus_of_rank0": (len(pinned) if pinned else None)},
            "full": full,
        }
        if gather_info is not None:
            out["gather"] = gather_info
        if full:
            rep["roofline"]["measured_hbm_read_GBps"] = hbm_read; rep["roofline"]["measured_hbm_copy_GBps"] = hbm_copy
            if "chi2_match" in extra:      # the parity gate travels with the number (flat, so that summaries of the line keep it)
                rep["roofline"]["chi2_max_rel_diff_vs_cpu"] = extra["chi2_match"]["max_rel_diff"]
                rep["roofline"]["chi2_match_ok"] = extra["chi2_match"]["ok"]
            out.update({
                "roofline": rep["roofline"],
                "cpu_baseline": cpu,
                "path_roofline": rep.get("path_roofline"),
                "stage_ms_per_step": rep["stage_ms_per_step"],
                "stage_launches_per_step": rep.get("stage_launches_per_step"),
                "counters_mean": rep["counters_mean"],
                "multi_gpu": multi,
                "gather_queueing": ({"from_inside_the_call": bool(getattr(w, "inside", False)),
                                     "host_ms_per_step_inside_the_callback": getattr(w, "cb_s", 0.0) / max(getattr(w, "k", 1), 1) * 1e3,
                                     "host_ms_per_step_in_the_library_calls": getattr(w, "call_s", 0.0) / max(getattr(w, "k", 1), 1) * 1e3} if (use_dist and not partition) else None),
            })
            if partition:
                out["partition"] = {"accepted_by_closer_thresholds_rank0": rep["accepted_by_closer_thresholds_rank0"], "keyframes_rank0": P,
                                    "max_translation_error_m_rank0": rep["max_translation_error_m_rank0"],
                                    "flat_cloud_bytes": int(w.flat_bytes) if use_dist else None,
                                    "broadcast_bytes_per_step": (int(w.flat_bytes) if w.pipeline else int(w.flat[0].numel())) if use_dist else None,
                                    "flat_buffer_bound_bytes": int(w.flat[0].numel()) if w.flat[0] is not None else None,
                                    "replica_roundtrip_on_rank0": bool(w.roundtrip), "pipelined": bool(w.pipeline),
                                    "pipeline": rep.get("pipeline")}
            out.update(extra)
        print(json.dumps(out))
    if use_dist:
        _progress(rank, world, "done; final barrier")
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
