"""Timing of the merged closure (PwnCloserWithMerger, pwn_tracker2) on one MI355X, next to the per-candidate closer on the same partition.

    python tools/bench_merged_closure.py [--partition 128] [--reps 20] [--warmup 3] [--seed 3]

Measures, on seeded VGA room frames (g2o_frontend_amd/synth.py), matcher at scale 1:
  * pwn_hip_project_merge_batch for 8 and 16 VGA clouds: the device time of its two kernels through the library's stage timers
    (pwn_hip_last_stage_ms: "project_depth_batch", "merge_depth_images"), median over the repetitions, and the bytes/s they achieve on
    the algorithmic traffic 12 * sum(M_k) + 4 N (2 n + 4): the points read, every plane cleared and read once, merged / weights read
    and written;
  * PwnCloserWithMerger.processPartition over the whole partition (clouds resident in the cache), host clock around the call -- every
    library call waits for its device work;
  * PwnMatcherBase.matchCloudsBatch of `current` against every cloud of the same partition, the same way.
The two closers compute different things (one alignment against a fused image / one alignment per candidate); the ratio is information.
Prints one JSON line.  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from g2o_frontend_amd import api, conf, synth      # noqa: E402

ROWS, COLS, K = 480, 640, synth.K_VGA
MIN_DISTANCE, MAX_DISTANCE = 0.01, 6.0


def algorithmic_bytes(point_counts, pixels):
    """(projection, fusion) bytes of one pwn_hip_project_merge_batch: 12 * sum(M_k) + 4 N n read and cleared / 4 N (n + 4) read and written"""
    n = len(point_counts)
    return 12 * sum(point_counts) + 4 * pixels * n, 4 * pixels * (n + 4)


def build_objects(ctx):
    cv, al = conf.VGA_CONF_CONVERTER, conf.VGA_CONF_ALIGNER
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]); proj.setMinDistance(MIN_DISTANCE); proj.setMaxDistance(MAX_DISTANCE)
    proj.setImageSize(ROWS, COLS)
    stats = api.StatsCalculatorIntegralImage()
    stats.setWorldRadius(cv["world_radius"]); stats.setMinImageRadius(cv["min_image_radius"]); stats.setMaxImageRadius(cv["max_image_radius"])
    stats.setMinPoints(cv["min_points"]); stats.setCurvatureThreshold(cv["stats_curvature_threshold"])
    pinfo, ninfo = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
    converter = api.DepthImageConverterIntegralImage(proj, stats, pinfo, ninfo)
    finder = api.CorrespondenceFinder()
    finder.setInlierDistanceThreshold(al["inlier_distance_threshold"]); finder.setInlierNormalAngularThreshold(al["inlier_normal_angular_threshold"])
    finder.setFlatCurvatureThreshold(al["flat_curvature_threshold"]); finder.setInlierCurvatureRatioThreshold(al["inlier_curvature_ratio_threshold"])
    finder.setImageSize(ROWS, COLS)
    lin = api.Linearizer(); lin.setInlierMaxChi2(al["inlier_max_chi2"]); lin.setRobustKernel(al["robust_kernel"])
    aligner = api.Aligner(ctx)
    aligner.setProjector(proj); aligner.setLinearizer(lin); aligner.setCorrespondenceFinder(finder)
    aligner.setOuterIterations(al["outer_iterations"]); aligner.setInnerIterations(al["inner_iterations"])
    matcher = api.PwnMatcherBase(aligner, converter)
    matcher.setScale(1)
    return proj, converter, aligner, matcher


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ms.append((time.perf_counter() - t) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--partition", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("bench_merged_closure: no HIP device (there is no CPU fallback)")
    n_part = max(16, a.partition)
    ctx = api.Context(device=0, max_rows=ROWS, max_cols=COLS, max_batch=n_part)
    proj, converter, aligner, matcher = build_objects(ctx)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float32)
    offset = np.eye(4, dtype=np.float32)
    poses = synth.trajectory(a.seed, n_part + 1, t_step=0.01, r_step_deg=0.5)
    cache = api.CloudCache(matcher, capacity=n_part + 1)
    nodes = []
    for k in range(n_part + 1):
        mm = synth.render_depth_mm(a.seed, poses[k], ROWS, COLS, K, hole_stream=k)
        cache.addFrame(k, mm.astype(np.float32) * np.float32(0.001), Km, offset)
        nodes.append(api.MapNode(k, poses[k], offset))
    current, others = nodes[0], nodes[1:]
    clouds = cache.getBatch([o.key for o in nodes])
    merger = api.Merger2(ctx, converter, matcher)
    closer = api.PwnCloserWithMerger(merger, cache)
    out = dict(rows=ROWS, cols=COLS, partition=n_part, reps=a.reps, warmup=a.warmup)

    # the two kernels, through the stage timers
    ctx.set_profiling(True)
    for n in (8, 16):
        sel = others[:n]
        trs = [closer.projectorTransform(o, current, o.sensorOffset) for o in sel]
        cl = [clouds[o.key] for o in sel]
        image = merger.zeros()
        t_proj, t_merge = [], []
        for rep in range(a.warmup + a.reps):
            merger.clear()
            image.zero()
            merger.projectMerge(image, cl, trs)
            if rep >= a.warmup:
                t_proj.append(ctx.stage_ms("project_depth_batch")[0]); t_merge.append(ctx.stage_ms("merge_depth_images")[0])
        bp, bm = algorithmic_bytes([len(c) for c in cl], ROWS * COLS)
        mp, mg = statistics.median(t_proj), statistics.median(t_merge)
        out["project_merge_%d" % n] = dict(
            points=sum(len(c) for c in cl), project_ms=mp, merge_ms=mg, project_ms_min=min(t_proj), project_ms_max=max(t_proj),
            merge_ms_min=min(t_merge), merge_ms_max=max(t_merge), project_bytes=bp, merge_bytes=bm,
            project_GBps=bp / (mp * 1e-3) / 1e9 if mp > 0 else None, merge_GBps=bm / (mg * 1e-3) / 1e9 if mg > 0 else None,
            both_GBps=(bp + bm) / ((mp + mg) * 1e-3) / 1e9 if mp + mg > 0 else None, overlaps=list(merger.overlaps))
    ctx.set_profiling(False)

    # the whole merged closure, and the per-candidate closer on the same partition
    relations = closer.processPartition(others, current)
    ms = timed(lambda: closer.processPartition(others, current), a.warmup, a.reps)
    out["merged_closure"] = dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), visited=len(merger.overlaps), relations=len(relations),
                                 accepted=closer.accepted, image_nonZeros=merger._result["image_nonZeros"] if merger._result else None)
    cur = clouds[current.key]
    part = [clouds[o.key] for o in others]
    reps_b = max(3, a.reps // 4)
    res = []
    ms = timed(lambda: res.append(matcher.matchCloudsBatch([cur] * len(part), part, offset, offset, Km, ROWS, COLS)), 1, reps_b)
    acc = api.PwnCloserAcceptance()
    out["match_clouds_batch"] = dict(pairs=len(part), reps=reps_b, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms),
                                     accepted=sum(1 for r in res[-1] if acc.accept(r)))
    out["ratio_batch_over_merged"] = out["match_clouds_batch"]["ms_median"] / out["merged_closure"]["ms_median"]
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
