"""What the closure records (include/pwn_hip.h: pwn_hip_closure_batch_records) cost on one MI355X, against the two routes that existed before.

    python tools/bench_closure_records.py [--pairs 128] [--reps 20] [--warmup 3] [--parent-lib PATH] [--out profiles/closure_records_bench.jsonl]

128 seeded VGA pairs (g2o_frontend_amd/synth.py), default sym6 clouds, converted once and kept (PwnMatcherBase.makeCloudBatch), the reference's VGA
configuration with ten outer iterations and the closer's kind of guess; two workloads: matcher scale 1 (480 x 640) and matcher scale 2 (240 x 320,
the reference's default).  Host clock around calls that end in the library's wait for the device, median of --reps calls, the routes timed
alternately in the same process:
  * `match_batch_records`: pwn_hip_match_batch_records, 72-word device records, no information matrix;
  * `closure_batch_records`: the new call, 128-word device records;
  * `align_batch_ex_and_pack`: the route that existed before for a relation WITH its information matrix -- pwn_hip_align_batch_ex(scores,
    statistics), whose 6x6 math runs in a host loop, then the 128-word records packed on the host (numpy, vectorised).  With --parent-lib it runs
    in a child process of the same session on THAT library (the parent commit's build), else on this tree's;
  * `pair_statistics`: k_pair_statistics alone, the stage timer of one profiled call of the new route (pwn_hip_last_stage_ms), with its launches.
One JSON line per workload.  Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from g2o_frontend_amd import synth      # noqa: E402
from bench_early_stop import ROWS, COLS, K, build_objects, closure_guesses, _render      # noqa: E402

NEW_SYMBOLS = ("pwn_hip_closure_batch_records", "pwn_hip_debug_statistics_eval")
STAT_WORDS = 88      # pwn_hip_align_statistics as 4-byte words: mean 6, omega 36, two ratios, H 36, b 6, error, inliers (int)


def pack_on_host(res, scores, stats, n, first_id=0):
    """[n, 128] closure records from the outputs of pwn_hip_align_batch_ex"""
    from g2o_frontend_amd import api, shard
    out = np.zeros((n, 128), np.float32)
    out[:, :64] = shard.pack_results_raw(np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=n), np.arange(first_id, first_id + n))
    sc = np.frombuffer(scores, np.int32).reshape(n, 4)
    out[:, 64] = sc[:, 0]; out[:, 65] = sc[:, 1]; out[:, 66] = sc[:, 2]; out[:, 67] = sc[:, 3].view(np.float32)
    st = np.frombuffer(stats, np.float32).reshape(n, STAT_WORDS)
    out[:, 72:108] = st[:, 6:42]; out[:, 108:114] = st[:, 0:6]; out[:, 114:116] = st[:, 42:44]
    out[:, 116] = st[:, 86]; out[:, 117] = st[:, 87].view(np.int32); out[:, 118] = 1.0
    return out


def run(args, only_existing):
    n = args.pairs
    seeds = list(range(n))
    with ProcessPoolExecutor(min(16, n)) as ex:                      # before the device is opened: the workers only render
        frames = list(ex.map(_render, seeds))
    from g2o_frontend_amd import _lib
    if only_existing:                                                # a library from before the feature: it lacks the two new symbols
        for name in NEW_SYMBOLS:
            _lib.PROTOTYPES.pop(name, None)
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import AlignResult, AlignStatistics, MatchResult
    assert C.sizeof(AlignStatistics) == 4 * STAT_WORDS
    ctx = api.Context(0, ROWS, COLS, max(n, 1))
    L = ctx._L
    converter, aligner = build_objects(api, ctx)
    matcher = api.PwnMatcherBase(aligner, converter)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float32); I = np.eye(4, dtype=np.float32)
    g = closure_guesses(seeds); gp = g.ctypes.data_as(C.c_void_p)
    lines = []
    for scale in (1, 2):
        matcher.setScale(scale)
        refs = matcher.makeCloudBatch(Km, I, [f[0] for f in frames], raw_scale=0.001)[0]
        curs = matcher.makeCloudBatch(Km, I, [f[1] for f in frames], raw_scale=0.001)[0]
        matcher._configure(I, I, Km, ROWS, COLS, None)
        p = aligner.params()
        hr = (C.c_void_p * n)(*[c.h for c in refs]); hc = (C.c_void_p * n)(*[c.h for c in curs])
        res = (AlignResult * n)(); scores = (MatchResult * n)(); stats = (AlignStatistics * n)()
        rec72 = ctx.upload(np.zeros((n, api.MATCH_RECORD_FLOATS), np.float32)); rec128 = ctx.upload(np.zeros((n, 128), np.float32))

        def match():
            ctx.check(L.pwn_hip_match_batch_records(ctx.h, C.byref(p), n, hr, hc, gp, 50.0, None, 0, None, None, C.c_void_p(rec72.data_ptr())))

        def closure():
            ctx.check(L.pwn_hip_closure_batch_records(ctx.h, C.byref(p), n, hr, hc, gp, 50.0, None, 0, None, None, None, C.c_void_p(rec128.data_ptr())))

        def existing():
            ctx.check(L.pwn_hip_align_batch_ex(ctx.h, C.byref(p), n, hr, hc, gp, res, 50.0, scores, stats))
            return pack_on_host(res, scores, stats, n)

        routes = (("align_batch_ex_and_pack", existing),) if only_existing else \
                 (("match_batch_records", match), ("closure_batch_records", closure), ("align_batch_ex_and_pack", existing))
        for _, call in routes:
            for _ in range(args.warmup):
                call()
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, call in routes:
                t0 = time.perf_counter(); call(); times[name].append((time.perf_counter() - t0) * 1e3)
        line = dict(workload="vga" if scale == 1 else "matcher_scale_2", pairs=n, rows=p.rows, cols=p.cols, omega_storage=ctx.omega_storage, outer_iterations=10,
                    reps=args.reps, library="PWN_HIP_LIB" if "PWN_HIP_LIB" in os.environ else "this tree")
        for name, t in times.items():
            line[name + "_ms"] = round(statistics.median(t), 3); line[name + "_min_max_ms"] = [round(min(t), 3), round(max(t), 3)]
        if not only_existing:
            same = np.array_equal(existing().view(np.uint32)[:, :119], rec128.numpy().reshape(n, 128).view(np.uint32)[:, :119])
            ctx.set_profiling(True); closure()
            ms, launches = ctx.stage_ms("pair_statistics"); lin_ms, _ = ctx.stage_ms("statistics")
            ctx.set_profiling(False)
            line.update(pair_statistics_ms=round(ms, 4), pair_statistics_launches=launches, statistics_pass_ms=round(lin_ms, 4),
                        pair_statistics_share_of_call=round(ms / line["closure_batch_records_ms"], 4),
                        host_packed_records_equal_device_records=bool(same))
        lines.append(line)
    ctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libpwn_hip.so built from the parent commit: the existing route is timed on it in a child process")
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
            ln["parent_library_align_batch_ex_and_pack_ms"] = ch["align_batch_ex_and_pack_ms"]
            ln["parent_library_align_batch_ex_and_pack_min_max_ms"] = ch["align_batch_ex_and_pack_min_max_ms"]
    for ln in lines:
        ref = ln.get("parent_library_align_batch_ex_and_pack_ms", ln["align_batch_ex_and_pack_ms"])
        if "closure_batch_records_ms" in ln:
            ln["closure_over_match_ms"] = round(ln["closure_batch_records_ms"] - ln["match_batch_records_ms"], 3)
            ln["closure_under_existing_route_ms"] = round(ref - ln["closure_batch_records_ms"], 3)
        print(json.dumps(ln), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
