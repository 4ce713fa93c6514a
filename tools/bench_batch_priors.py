"""What SE(3) priors cost a candidate batch on one MI355X: the device-resident loop with priors (include/pwn_hip.h: pwn_hip_align_batch_priors)
against the same batch without priors and against one single call per pair (pwn_hip_align_with_priors_ex: one pair of the batch call on this
tree's library; on a library from before that, the loop the host drove).

    python tools/bench_batch_priors.py [--pairs 128] [--reps 20] [--warmup 3] [--parent-lib PATH] [--out profiles/batch_priors_bench.jsonl]

128 seeded VGA pairs (g2o_frontend_amd/synth.py), default sym6 clouds, converted once and kept (PwnMatcherBase.makeCloudBatch, matcher scale 2:
240 x 320, the reference's default), the reference's VGA configuration with ten outer iterations and the closer's kind of guess; per pair one
absolute and one relative prior, in that order (pwn_tracker2 adds the IMU prior, then the odometry prior), means a few centimetres off the pair's
pose.  Host clock around calls that end in the library's wait for the device, median of --reps calls, the routes timed alternately:
  (a) `closure_batch_records`: pwn_hip_closure_batch_records, 128-word device records, no priors;
  (b) `batch_priors_closure`: the new call with closure records and the priors;
  (c) `single_call_loop`: per pair pwn_hip_align_with_priors_ex(statistics) + pwn_hip_match_score on this tree's library -- and with --parent-lib
      in a child process of the same session on THAT library (the parent commit's build), where the route keeps its name there, `host_driven_loop`;
  (d) one VGA pair (480 x 640): `one_pair_single_call` (`one_pair_host_driven` in the child) against `one_pair_batch_priors` (n = 1 of the batch
      call, results + statistics + score);
  `prior_terms`: k_prior_terms alone, the stage timer of one profiled call of (b), with its launches.
Both processes feed what the per-pair route returns -- every pwn_hip_align_result with total_time_ms zeroed, every pwn_hip_align_statistics, every
pwn_hip_match_result -- into a CRC32 per workload (`per_pair_route_crc32`); with --parent-lib the line says whether the two are equal
(`single_call_equals_parent_host_driven_loop`).  One JSON line per workload.  Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from g2o_frontend_amd import synth      # noqa: E402
from bench_early_stop import ROWS, COLS, K, build_objects, closure_guesses, _render      # noqa: E402

NEW_SYMBOLS = ("pwn_hip_align_batch_priors", "pwn_hip_prior_terms", "pwn_hip_debug_prior_terms_eval")
INFO = (np.diag([4e5, 4e5, 4e5, 2e6, 2e6, 2e6]) + 1e4).astype(np.float32)
REFT = synth.v2t(np.array([0.02, 0.01, -0.01, 0.0, 0.01, 0.0]))


def priors_of(seed):
    """[absolute, relative] of a pair, as (kind, mean, referenceTransform, information)"""
    P = synth.pair_pose(seed)
    a = (1, (REFT @ P @ synth.v2t(np.array([0.02, 0.01, -0.03, 0.0, 0.01, -0.01]))).astype(np.float32), REFT.astype(np.float32), (INFO * 0.5).astype(np.float32))
    r = (0, (P @ synth.v2t(np.array([-0.01, -0.02, 0.02, 0.005, 0.01, 0.0]))).astype(np.float32), np.eye(4, dtype=np.float32), INFO)
    return [a, r]


def _median_line(times):
    out = {}
    for name, t in times.items():
        out[name + "_ms"] = round(statistics.median(t), 3); out[name + "_min_max_ms"] = [round(min(t), 3), round(max(t), 3)]
    return out


def run(args, only_existing):
    n = args.pairs
    seeds = list(range(n))
    with ProcessPoolExecutor(min(16, n)) as ex:                      # before the device is opened: the workers only render
        frames = list(ex.map(_render, seeds))
    from g2o_frontend_amd import _lib
    if only_existing:                                                # a library from before the feature: it lacks the new symbols
        for name in NEW_SYMBOLS:
            _lib.PROTOTYPES.pop(name, None)
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import AlignResult, AlignStatistics, MatchResult, PairPriors, Prior
    ctx = api.Context(0, ROWS, COLS, max(n, 1))
    L = ctx._L
    converter, aligner = build_objects(api, ctx)
    matcher = api.PwnMatcherBase(aligner, converter)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float32); I = np.eye(4, dtype=np.float32)
    g = closure_guesses(seeds)
    arr = (Prior * (2 * n))()
    for i, s in enumerate(seeds):
        for j, (kind, mean, reft, info) in enumerate(priors_of(s)):
            q = arr[2 * i + j]
            q.kind = kind; api._set(q.mean, mean, 4); api._set(q.reference_transform, reft, 4); api._set(q.information, info, 6)
    first = np.arange(0, 2 * n + 1, 2, dtype=np.int32)
    pp = PairPriors(first.ctypes.data_as(C.POINTER(C.c_int)), C.cast(arr, C.POINTER(Prior)))
    lines = []
    for scale, m in ((2, n), (1, 1)):
        matcher.setScale(scale)
        refs = matcher.makeCloudBatch(Km, I, [f[0] for f in frames[:m]], raw_scale=0.001)[0]
        curs = matcher.makeCloudBatch(Km, I, [f[1] for f in frames[:m]], raw_scale=0.001)[0]
        matcher._configure(I, I, Km, ROWS, COLS, None)
        p = aligner.params()
        per_pair = []
        for i in range(m):                                           # the single call takes its guess from the parameters
            q = aligner.params(); C.memmove(q.initial_guess, g[i].ctypes.data, 64); per_pair.append(q)
        hr = (C.c_void_p * m)(*[c.h for c in refs]); hc = (C.c_void_p * m)(*[c.h for c in curs])
        gp = g[:m].ctypes.data_as(C.c_void_p)
        res = (AlignResult * m)(); scores = (MatchResult * m)(); stats = (AlignStatistics * m)()
        rec128 = ctx.upload(np.zeros((m, 128), np.float32))

        def closure():
            ctx.check(L.pwn_hip_closure_batch_records(ctx.h, C.byref(p), m, hr, hc, gp, 50.0, None, 0, None, None, None, C.c_void_p(rec128.data_ptr())))

        def batch_priors():
            ctx.check(L.pwn_hip_align_batch_priors(ctx.h, C.byref(p), m, hr, hc, gp, C.byref(pp), 50.0, None, 0, None, None, None,
                                                   C.c_void_p(rec128.data_ptr()), 128))

        def one_pair_batch_priors():
            ctx.check(L.pwn_hip_align_batch_priors(ctx.h, C.byref(p), m, hr, hc, gp, C.byref(pp), 50.0, None, 0, res, scores, stats, None, 0))

        def single_calls():
            for i in range(m):
                ctx.check(L.pwn_hip_align_with_priors_ex(ctx.h, C.byref(per_pair[i]), hr[i], hc[i], 2, C.byref(arr[2 * i]), C.byref(res[i]), C.byref(stats[i])))
                ctx.check(L.pwn_hip_match_score(ctx.h, 50.0, C.byref(scores[i])))

        single = "host_driven" if only_existing else "single_call"      # what the per-pair route is on the library it runs on
        if scale == 2:
            routes = ((single + "_loop", single_calls),) if only_existing else \
                     (("closure_batch_records", closure), ("batch_priors_closure", batch_priors), (single + "_loop", single_calls))
        else:
            routes = (("one_pair_" + single, single_calls),) if only_existing else \
                     (("one_pair_" + single, single_calls), ("one_pair_batch_priors", one_pair_batch_priors))
        for _, call in routes:
            for _ in range(args.warmup):
                call()
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, call in routes:
                t0 = time.perf_counter(); call(); times[name].append((time.perf_counter() - t0) * 1e3)
        line = dict(workload="matcher_scale_2" if scale == 2 else "one_vga_pair", pairs=m, rows=p.rows, cols=p.cols, omega_storage=ctx.omega_storage,
                    outer_iterations=p.outer_iterations, priors_per_pair=2, reps=args.reps, library="PWN_HIP_LIB" if "PWN_HIP_LIB" in os.environ else "this tree")
        line.update(_median_line(times))
        # everything the per-pair route returns, for the comparison across the two libraries
        single_calls()
        r = np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=m).copy(); r["total_time_ms"] = 0
        line["per_pair_route_crc32"] = zlib.crc32(bytes(scores), zlib.crc32(bytes(stats), zlib.crc32(r.tobytes())))
        if not only_existing:
            # the two routes of this library return the same bits (T of every pair)
            want = r["T"].copy()
            res2 = (AlignResult * m)()
            ctx.check(L.pwn_hip_align_batch_priors(ctx.h, C.byref(p), m, hr, hc, gp, C.byref(pp), 50.0, None, 0, res2, None, None, None, 0))
            same = np.array_equal(want.view(np.uint32), np.frombuffer(res2, dtype=api.ALIGN_RESULT_DTYPE, count=m)["T"].view(np.uint32))
            ctx.set_profiling(True); (batch_priors if scale == 2 else one_pair_batch_priors)()
            ms, launches = ctx.stage_ms("prior_terms"); solve_ms, solve_launches = ctx.stage_ms("solve")
            ctx.set_profiling(False)
            line.update(prior_terms_ms=round(ms, 4), prior_terms_launches=launches, prior_terms_us_per_launch=round(1e3 * ms / max(launches, 1), 3),
                        solve_ms=round(solve_ms, 4), solve_launches=solve_launches, batch_priors_equals_single_call_loop=bool(same))
        lines.append(line)
    ctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libpwn_hip.so built from the parent commit: the per-pair route is timed on it in a child process, and its results compared")
    ap.add_argument("--existing-route-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = run(args, args.existing_route_only)
    if args.parent_lib and not args.existing_route_only:
        env = dict(os.environ, PWN_HIP_LIB=os.path.abspath(args.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--pairs", str(args.pairs), "--reps", str(args.reps), "--warmup", str(args.warmup),
                            "--existing-route-only"], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("child on the parent library failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        child = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        for ln, ch in zip(lines, child):
            for k, v in ch.items():
                if k.endswith("_ms") and ("host_driven" in k):
                    ln["parent_library_" + k] = v
            ln["parent_library_per_pair_route_crc32"] = ch["per_pair_route_crc32"]
            ln["single_call_equals_parent_host_driven_loop"] = ln["per_pair_route_crc32"] == ch["per_pair_route_crc32"]
    for ln in lines:
        if "batch_priors_closure_ms" in ln:
            ref = ln.get("parent_library_host_driven_loop_ms", ln["single_call_loop_ms"])
            ln["priors_over_no_priors_ms"] = round(ln["batch_priors_closure_ms"] - ln["closure_batch_records_ms"], 3)
            ln[("host_driven" if args.parent_lib else "single_call") + "_loop_over_batch_priors"] = round(ref / ln["batch_priors_closure_ms"], 2)
        if "one_pair_batch_priors_ms" in ln:
            ref = ln.get("parent_library_one_pair_host_driven_ms", ln["one_pair_single_call_ms"])
            ln["one_pair_" + ("host_driven" if args.parent_lib else "single_call") + "_over_batch_priors"] = round(ref / ln["one_pair_batch_priors_ms"], 2)
        print(json.dumps(ln), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
