"""Timing of scene-ready batch conversion (pwn_hip_convert_batch_ex: Stats and sensor-noise Gaussians inside the batch submission) on one MI355X.

    python tools/bench_scene_ready.py [--frames 128] [--reps 20] [--warmup 3] [--parent-lib build/variants/base.so] [--out profiles/scene_ready_bench.jsonl]

128 VGA uint16 frames resident on the device (16 seeded room frames of g2o_frontend_amd/synth.py, each eight times), converted unscaled and at step 2
(DepthImage_scale in front, camera matrix halved).  Host clock around each call, which ends in its one wait for the device; median, minimum and
maximum over the repetitions.  Per configuration one JSON line:
  * `lean`: the existing batch call (pwn_hip_convert_batch_u16[_scaled]), in three blocks of repetitions; `lean_spread_ms` is the largest difference
    between two block medians, the run-to-run spread of this session.  `lean_ex_null`: the same through the new entry point without extras.
    `parent_lean` (with --parent-lib: a library built from the parent commit, tools/ab_build.py): the same call in a child process of this
    session, run before and again after this process's own measurements (`parent_lean_after`), and between those two this tree's library
    through the same child process (`lean_child`: same program, same process history, only the library differs).  The lean path is not
    supposed to move: `lean_child` should lie between the parent's two, give or take the spread.
  * `keep_stats`, `gaussians`, `both`: the call with the extras.
  * `per_frame`: the route that existed for the same frames -- per frame pwn_hip_convert(keep_stats = 1) and pwn_hip_cloud_gaussians on the float
    image (made beforehand, on the device, outside the timed region): 4 n launches more and n host waits.
  * `gaussian_kernel`: k_gaussians_batch alone, from the library's stage timer (events around the launches, summed over the sub-batches; the
    context on one stream for these runs, so that nothing else runs between the events), with every lane storing its own 96-byte record
    (`per_lane`) and staged through LDS (`staged`); `call_per_lane` / `call_staged`: the whole call with Gaussians in either form, streams as
    usual; `bytes`: 100 per point written, 4 of index and 2 (raw) or 4 (down-sampled float) of depth per pixel read; `floor_ms`: those bytes over the copy rate this GPU delivered in the same process
    (pwn_hip_measure_hbm).
Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from g2o_frontend_amd import _lib      # noqa: E402

ROWS, COLS = 480, 640
RAW_SCALE, COV = 0.001, 0.01
F = np.float32
DISTINCT = 16


def summary(ms):
    return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ms.append((time.perf_counter() - t) * 1e3)
    return ms


def setup(frames_n, seed):
    from g2o_frontend_amd import api, conf, synth
    ctx = api.Context(device=0, max_rows=ROWS, max_cols=COLS, max_batch=frames_n)
    poses = synth.trajectory(seed, DISTINCT, t_step=0.08, r_step_deg=4.0)
    distinct = [synth.render_depth_mm(seed, poses[k], ROWS, COLS, synth.K_VGA, hole_stream=k) for k in range(DISTINCT)]
    frames = np.stack([distinct[i % DISTINCT] for i in range(frames_n)]).astype(np.uint16)
    dev = ctx.upload(frames)
    return api, conf, synth, ctx, frames, dev


def params(api, conf, synth, step):
    cv = conf.VGA_CONF_CONVERTER
    s = max(step, 1)
    K = synth.K_VGA
    proj = api.PinholePointProjector()
    Km = (np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], F) * (F(1.0) / F(s))).astype(F); Km[2, 2] = 1.0
    proj.setCameraMatrix(Km); proj.setMinDistance(cv["min_distance"]); proj.setMaxDistance(cv["max_distance"])
    stats = api.StatsCalculatorIntegralImage()
    stats.setWorldRadius(cv["world_radius"]); stats.setMinImageRadius(cv["min_image_radius"] // s); stats.setMaxImageRadius(cv["max_image_radius"] // s)
    stats.setMinPoints(cv["min_points"] // (s * s)); stats.setCurvatureThreshold(cv["stats_curvature_threshold"])
    converter = api.DepthImageConverterIntegralImage(proj, stats, api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator())
    return converter.params(None), proj


def lean_call(ctx, p, ptrs, handles, n, step):
    if step:
        ctx.check(ctx._L.pwn_hip_convert_batch_u16_scaled(ctx.h, C.byref(p), ptrs, RAW_SCALE, n, ROWS, COLS, step, COV, handles))
    else:
        ctx.check(ctx._L.pwn_hip_convert_batch_u16(ctx.h, C.byref(p), ptrs, RAW_SCALE, n, ROWS, COLS, handles))


def lean_only(a):
    """the existing call alone, with whatever library PWN_HIP_LIB names (a parent build lacks the new symbols: their prototypes are dropped)"""
    L = C.CDLL(_lib.LIB_PATH)
    for name in [k for k in _lib.PROTOTYPES if not hasattr(L, k)]:
        del _lib.PROTOTYPES[name]
    api, conf, synth, ctx, frames, dev = setup(a.frames, a.seed)
    out = {}
    for step in (0, 2):
        p, _ = params(api, conf, synth, step)
        s = max(step, 1)
        clouds = [api.Cloud(ctx, (ROWS // s) * (COLS // s)) for _ in range(a.frames)]
        ptrs = (C.c_void_p * a.frames)(*[dev.frame(i).data_ptr() for i in range(a.frames)]); handles = (C.c_void_p * a.frames)(*[c.h for c in clouds])
        blocks = [timed(lambda: lean_call(ctx, p, ptrs, handles, a.frames, step), a.warmup, a.reps) for _ in range(3)]
        out[str(step)] = dict(summary(sum(blocks, [])), block_medians=[statistics.median(b) for b in blocks])
        del clouds
    print(json.dumps(out))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit: its lean call is timed in a child process first")
    ap.add_argument("--lean-only", action="store_true", help="time the existing call only and print one JSON object (what the child process runs)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if a.lean_only:
        return lean_only(a)
    def child_run(lib):      # while this process has no context open: one process times at a time
        env = dict(os.environ, PWN_HIP_LIB=os.path.abspath(lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lean-only", "--frames", str(a.frames), "--reps", str(a.reps), "--warmup", str(a.warmup),
                            "--seed", str(a.seed)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit("bench_scene_ready: the child process's run failed:\n" + r.stderr[-800:])
        return json.loads(r.stdout.strip().splitlines()[-1])
    parent = child_run(a.parent_lib) if a.parent_lib else None
    api, conf, synth, ctx, frames, dev = setup(a.frames, a.seed)
    if api.device_count() < 1:
        raise SystemExit("bench_scene_ready: no HIP device (there is no CPU fallback)")
    read_GBps, copy_GBps = ctx.measure_hbm()
    n = a.frames
    lines = []
    for step in (0, 2):
        p, proj = params(api, conf, synth, step)
        s = max(step, 1)
        orows, ocols = ROWS // s, COLS // s
        clouds = [api.Cloud(ctx, orows * ocols) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[dev.frame(i).data_ptr() for i in range(n)]); handles = (C.c_void_p * n)(*[c.h for c in clouds])

        def ex_call(ex):
            ctx.check(ctx._L.pwn_hip_convert_batch_ex(ctx.h, C.byref(p), ptrs, 1, RAW_SCALE, n, ROWS, COLS, step, COV, None if ex is None else C.byref(ex), handles))
        blocks = [timed(lambda: lean_call(ctx, p, ptrs, handles, n, step), a.warmup, a.reps) for _ in range(3)]
        meds = [statistics.median(b) for b in blocks]
        line = dict(bench="scene_ready", frames=n, rows=ROWS, cols=COLS, step=step, reps=a.reps, warmup=a.warmup,
                    lean=dict(summary(sum(blocks, [])), block_medians=meds), lean_spread_ms=max(meds) - min(meds),
                    lean_ex_null=summary(timed(lambda: ex_call(None), a.warmup, a.reps)))
        if parent is not None:
            line["parent_lean"] = parent[str(step)]
            line["lean_minus_parent_ms"] = line["lean"]["ms_median"] - parent[str(step)]["ms_median"]
            pm = parent[str(step)]["block_medians"]
            line["parent_spread_ms"] = max(pm) - min(pm)
        for name, ks, ga in (("keep_stats", 1, 0), ("gaussians", 0, 1), ("both", 1, 1)):
            ex = _lib.ConvertExtras(ks, ga, proj.baseline(), proj.alpha())
            line[name] = summary(timed(lambda: ex_call(ex), a.warmup, a.reps))
        points = [c.size() for c in clouds]
        assert all(c.numGaussians() == c.size() for c in clouds)
        # the kernel alone, in both store forms (the stage timer's events around its launches)
        ex = _lib.ConvertExtras(0, 1, proj.baseline(), proj.alpha())
        calls = {}
        for form, label in ((0, "call_per_lane"), (1, "call_staged")):
            ctx.check(ctx._L.pwn_hip_debug_set_gaussian_stores(ctx.h, form))
            calls[label] = summary(timed(lambda: ex_call(ex), a.warmup, a.reps))
        ctx.set_profiling(True)
        ctx.set_concurrency(1)
        kern = {}
        for form, label in ((0, "per_lane"), (1, "staged")):
            ctx.check(ctx._L.pwn_hip_debug_set_gaussian_stores(ctx.h, form))
            ms = []
            for rep in range(a.warmup + a.reps):
                ex_call(ex)
                if rep >= a.warmup:
                    ms.append(ctx.stage_ms("gaussians")[0])
            kern[label] = dict(summary(ms), launches=ctx.stage_ms("gaussians")[1])
        ctx.check(ctx._L.pwn_hip_debug_set_gaussian_stores(ctx.h, -1))
        ctx.set_profiling(False)
        ctx.set_concurrency(4)
        nbytes = 100 * sum(points) + (4 + (4 if step else 2)) * orows * ocols * n
        line["gaussian_kernel"] = dict(kern, **calls, points=sum(points), bytes=nbytes, floor_ms=nbytes / (copy_GBps * 1e9) * 1e3)
        # the per-frame route on the same frames: the float image on the device beforehand
        host = [np.ascontiguousarray(frames[i]) for i in range(min(n, DISTINCT))]
        flt = ctx.DepthImage_scale_batch(host, step, COV, raw_scale=RAW_SCALE) if step else [ctx.DepthImage_convert_16UC1_to_32FC1(f, RAW_SCALE) for f in host]
        fdev = ctx.upload(np.stack([flt[i % DISTINCT] for i in range(n)]).astype(F))
        fptr = [C.c_void_p(fdev.frame(i).data_ptr()) for i in range(n)]

        def per_frame():
            for i in range(n):
                ctx.check(ctx._L.pwn_hip_convert(ctx.h, C.byref(p), fptr[i], orows, ocols, clouds[i].h, None, None, 1))
                ctx.check(ctx._L.pwn_hip_cloud_gaussians(ctx.h, C.byref(p), fptr[i], orows, ocols, clouds[i].h, proj.baseline(), proj.alpha()))
        line["per_frame"] = summary(timed(per_frame, 1, a.reps))
        assert [c.size() for c in clouds] == points
        line["per_frame_over_both"] = line["per_frame"]["ms_median"] / line["both"]["ms_median"]
        line.update(hbm_read_GBps=read_GBps, hbm_copy_GBps=copy_GBps)
        lines.append(line)
        fdev.free()
        del clouds
    dev.free()
    ctx.close()
    if a.parent_lib:
        same, after = child_run(_lib.LIB_PATH), child_run(a.parent_lib)
        for line in lines:
            line["lean_child"] = same[str(line["step"])]
            line["parent_lean_after"] = after[str(line["step"])]
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
