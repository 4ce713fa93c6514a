#!/usr/bin/env python3
"""Timing of the batched makeCloud data path at 1 / step resolution (docs/experiments.md): 64 VGA uint16 frames resident on the device, default
sym6 clouds, steps 2 and 4,

  (a) what a caller did before pwn_hip_convert_batch_u16_scaled existed: per frame pwn_hip_depth_u16_to_f32 + pwn_hip_convert_scaled,
      each call waiting for the host;
  (b) one pwn_hip_convert_batch_u16_scaled.

Both are warmed up, then timed alternately (a, b, a, b, ...) with a host clock around calls that end in a device synchronise; the median and
the spread of each are reported.  In a run of its own with stage timing on: the box kernel's time (pwn_hip_last_stage_ms "depth_scale") and
the bytes it reads and writes over that time, as a fraction of the streaming-read rate pwn_hip_measure_hbm finds on the same device.
Prints one JSON line per step.

  python tools/bench_scaled_batch.py [--frames 64] [--repeats 20] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS, COV, RAW_SCALE = 480, 640, 0.01, 0.001


def converter(K):
    from g2o_frontend_amd import api, conf
    c = conf.QVGA4_CONF_CONVERTER
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    proj.setMinDistance(c["min_distance"]); proj.setMaxDistance(c["max_distance"])
    stats = api.StatsCalculatorIntegralImage()
    stats.setWorldRadius(c["world_radius"]); stats.setMinImageRadius(c["min_image_radius"]); stats.setMaxImageRadius(c["max_image_radius"])
    stats.setMinPoints(c["min_points"]); stats.setCurvatureThreshold(c["stats_curvature_threshold"])
    pinfo, ninfo = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
    pinfo.setCurvatureThreshold(c["point_info_curvature_threshold"]); ninfo.setCurvatureThreshold(c["normal_info_curvature_threshold"])
    return api.DepthImageConverterIntegralImage(proj, stats, pinfo, ninfo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from g2o_frontend_amd import api, synth
    n = args.frames
    ctx = api.Context(0, ROWS, COLS, max(n, 1))
    L = ctx._L
    read_gbps, _ = ctx.measure_hbm()
    poses = synth.trajectory(11, n)
    frames = [ctx.upload(synth.render_depth_mm(11, poses[k], ROWS, COLS, synth.K_VGA, hole_stream=k)) for k in range(n)]
    ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in frames])
    depth = ctx.upload(np.zeros((ROWS, COLS), np.float32))
    for step in (2, 4):
        p = converter(synth.scaled_K(synth.K_VGA, step)).params(None)
        N = (ROWS // step) * (COLS // step)
        clouds = [api.Cloud(ctx, N) for _ in range(n)]
        handles = (C.c_void_p * n)(*[c.h for c in clouds])

        def per_frame():
            for k in range(n):
                ctx.check(L.pwn_hip_depth_u16_to_f32(ctx.h, C.c_void_p(frames[k].data_ptr()), C.c_void_p(depth.data_ptr()), ROWS * COLS, RAW_SCALE))
                ctx.check(L.pwn_hip_convert_scaled(ctx.h, C.byref(p), C.c_void_p(depth.data_ptr()), ROWS, COLS, step, COV, clouds[k].h))

        def batch():
            ctx.check(L.pwn_hip_convert_batch_u16_scaled(ctx.h, C.byref(p), ptrs, RAW_SCALE, n, ROWS, COLS, step, COV, handles))

        per_frame()
        sizes = [c.size() for c in clouds]
        batch()
        assert [c.size() for c in clouds] == sizes and min(sizes) > 0, "the two paths disagree on the clouds' sizes"
        for _ in range(args.warmup):
            per_frame(); batch()
        ta, tb = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter(); per_frame(); t1 = time.perf_counter(); batch(); t2 = time.perf_counter()
            ta.append((t1 - t0) * 1e3); tb.append((t2 - t1) * 1e3)
        # the box kernel alone, in calls of their own with stage timing on
        ctx.set_profiling(True)
        ks = []
        for _ in range(max(3, args.repeats // 2)):
            batch()
            ms, launches = ctx.stage_ms("depth_scale")
            ks.append(ms)
        ctx.set_profiling(False)
        moved = n * (ROWS // step * step) * (COLS // step * step) * 2 + n * N * 4      # bytes the kernel reads and writes
        kms = statistics.median(ks)
        a, b = statistics.median(ta), statistics.median(tb)
        print(json.dumps(dict(step=step, frames=n, per_frame_calls_ms=round(a, 3), per_frame_calls_min_max_ms=[round(min(ta), 3), round(max(ta), 3)],
                              batch_call_ms=round(b, 3), batch_call_min_max_ms=[round(min(tb), 3), round(max(tb), 3)], ratio=round(a / b, 2),
                              depth_scale_kernel_ms=round(kms, 4), depth_scale_launches=launches, depth_scale_bytes=moved,
                              depth_scale_gbps=round(moved / (kms * 1e-3) / 1e9, 1) if kms > 0 else None, hbm_read_gbps=round(read_gbps, 1),
                              fraction_of_hbm_read=round(moved / (kms * 1e-3) / 1e9 / read_gbps, 3) if kms > 0 and read_gbps > 0 else None)), flush=True)
        del clouds
    ctx.close()


if __name__ == "__main__":
    main()
