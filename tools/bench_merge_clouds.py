"""Timing of the cloud-level fusion (Merger2::merge through PwnMerger::mergeNodeList, pwn_tracker2) on one MI355X.

    python tools/bench_merge_clouds.py [--reps 20] [--warmup 3] [--seed 3] [--out profiles/merge_clouds_bench.jsonl]

One nine-cloud list (listSize 8, as pwn_slam_gui_merger_gaze_pwn_merger.conf sets it) of seeded VGA room frames (g2o_frontend_amd/synth.py),
matcher at scale 1 (480 x 640 clouds) and at scale 2 (240 x 320).  Per scale, one JSON line:
  * `one_call`: pwn_hip_merge_clouds of the nine resident clouds into an empty total whose arrays exist -- host clock around the call,
    which ends in its one wait for the device; median, minimum and maximum over the repetitions; `mirror`: Merger2.clearCloud + mergeBatch,
    which allocates the total and its weights per list on top of that;
  * `composed`, for information: the same fusion from the calls that existed before -- pwn_hip_project per cloud and per total, Cloud.add
    into a scratch cloud for the transformed arrays, downloads, the decisions and the fuse in numpy, the upload of the grown total;
    it leaves the device 2 n times per list.  Its point count and appended / fused counters are checked against the one call's;
  * `bytes`: what the kernels of the one call have to move, computed from the shapes and the measured counters (algorithmic_bytes), and
    `floor_ms`: those bytes over the streaming-read rate this GPU delivered in the same process (pwn_hip_measure_hbm).  The ratio
    one_call / floor says how far the call is from its traffic; at these sizes the call is made of launches (ten per cloud), not of traffic.
Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
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
LIST = 9
F = np.float32


def algorithmic_bytes(pixels, source_points, total_before, appended, fused, omega_floats=6, gaussians=False):
    """bytes of one pwn_hip_merge_clouds list, per cloud i: the two z-buffers cleared (16 N), both clouds' points read and one 8-byte atomic
    per point (20 (M_i + total_i)), the decisions (16 N read, 4 N flags written, 40 per fuse: point and weight read and written), the scan
    (flags read, offsets written, read and written again: 16 N), the appends (flags and offsets read: 8 N; per appended point the z word,
    the source record read and the total's record and weight written)"""
    record = 12 + 16 + 4 * omega_floats + 36 + 64 + (100 if gaussians else 0)          # xyz, normal + curvature, Omega_p, Omega_n, Stats (, Gaussian + flags)
    b = 0
    for m, t, a, f in zip(source_points, total_before, appended, fused):
        b += 16 * pixels + 20 * (m + t) + 20 * pixels + 40 * f + 16 * pixels + 8 * pixels + a * (8 + 2 * record + 4)
    return b


def build_objects(ctx, scale):
    cv = conf.VGA_CONF_CONVERTER
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]); proj.setMinDistance(cv["min_distance"]); proj.setMaxDistance(cv["max_distance"])
    proj.setImageSize(ROWS, COLS)
    stats = api.StatsCalculatorIntegralImage()
    stats.setWorldRadius(cv["world_radius"]); stats.setMinImageRadius(cv["min_image_radius"] // scale); stats.setMaxImageRadius(cv["max_image_radius"] // scale)
    stats.setMinPoints(cv["min_points"] // (scale * scale)); stats.setCurvatureThreshold(cv["stats_curvature_threshold"])
    pinfo, ninfo = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
    converter = api.DepthImageConverterIntegralImage(proj, stats, pinfo, ninfo)
    aligner = api.Aligner(ctx)
    aligner.setProjector(proj)
    matcher = api.PwnMatcherBase(aligner, converter)
    matcher.setScale(scale)
    return proj, converter, matcher


def composed(ctx, proj, clouds, transforms, offset):
    """Merger2::merge of the list from pwn_hip_project, Cloud.add, downloads, numpy and uploads -> (points, appended[n], fused[n])"""
    keys = ("points", "normals", "curvature", "omega_p", "omega_n")
    tot = None
    w = np.zeros(0, F)
    appended, fused = [], []
    rows, cols = proj.imageRows(), proj.imageCols()
    mn, mx = F(proj.minDistance()), F(proj.maxDistance())
    cap = sum(c.size() for c in clouds)
    tot_gpu = api.Cloud(ctx, max(1, cap))
    for c, T in zip(clouds, transforms):
        proj.setTransform(offset)
        idx_c, d = proj.project(c)
        Ttot = api.iso_mul(T, offset)
        if tot is not None and len(tot["points"]):
            tot_gpu.upload(*[tot[k] for k in keys])
            proj.setTransform(Ttot)
            idx_t, dep_t = proj.project(tot_gpu)
        else:
            idx_t, dep_t = np.full((rows, cols), -1, np.int32), np.zeros((rows, cols), F)
        scratch = api.Cloud(ctx, max(1, c.size()))
        scratch.add(c, T)                                         # the transformed arrays (Cloud::add skips the identity; a timing, not a parity run)
        a = scratch.arrays()
        proj.setTransform(Ttot)
        iKRt = proj.matrices()[1]
        with np.errstate(all="ignore"):
            d64 = d.astype(np.float64)
            sel = (d64 > 0.2) & (d64 < 100)
            new = sel & (idx_t < 0)
            delta = d - dep_t
            near = np.abs(delta).astype(np.float64) < .15
            fuse = sel & ~new & near & ~((d < mn) | (d > mx))
            app = new | (sel & ~new & ~near & (delta.astype(np.float64) < -.3))
            rr, cc = np.nonzero(fuse)
            dd = d[rr, cc]; it = idx_t[rr, cc]
            x, y = cc.astype(F) * dd, rr.astype(F) * dd
            peso = F(1) / dd
            if len(it):
                pt = w[it]; somma = pt + peso
                for k in range(3):
                    p = ((iKRt[k, 0] * x + iKRt[k, 1] * y) + iKRt[k, 2] * dd) + iKRt[k, 3] * F(1)
                    tot["points"][it, k] = (tot["points"][it, k] * pt + p * peso) / somma
                w[it] = somma
            rr, cc = np.nonzero(app)
            rows_src = idx_c[rr, cc]
            new_rows = {k: a[k][rows_src] for k in keys}
            tot = new_rows if tot is None else {k: np.concatenate([tot[k], new_rows[k]]) for k in keys}
            w = np.concatenate([w, (F(1) / d[rr, cc]).astype(F)])
        appended.append(int(app.sum())); fused.append(int(fuse.sum()))
    tot_gpu.upload(*[tot[k] for k in keys])
    ctx.synchronize()
    return len(tot["points"]), appended, fused


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ms.append((time.perf_counter() - t) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("bench_merge_clouds: no HIP device (there is no CPU fallback)")
    ctx = api.Context(device=0, max_rows=ROWS, max_cols=COLS, max_batch=LIST)
    read_GBps, copy_GBps = ctx.measure_hbm()
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], F)
    offset = np.eye(4, dtype=F)
    poses = synth.trajectory(a.seed, LIST, t_step=0.08, r_step_deg=4.0)
    frames = [synth.render_depth_mm(a.seed, poses[k], ROWS, COLS, K, hole_stream=k).astype(F) * F(0.001) for k in range(LIST)]
    nodes = [api.MapNode(k, poses[k], offset) for k in range(LIST)]
    lines = []
    for scale in (1, 2):
        proj, converter, matcher = build_objects(ctx, scale)
        clouds = matcher.makeCloudBatch(Km, offset, frames)[0]
        rows, cols = proj.imageRows(), proj.imageCols()
        trs = [api.PwnMerger.nodeTransform(nodes[0], o) for o in nodes]
        merger = api.Merger2(ctx, converter, matcher)

        # the call alone: a fresh total per repetition, created and given its scene arrays (a list of one empty cloud allocates them and merges
        # nothing) outside the timed region; one weight buffer, which needs no clearing (appends write their entry before a fuse reads it)
        cap = sum(c.size() for c in clouds)
        weights = api.DeviceBuffer(ctx, np.zeros(cap, F))
        empty = api.Cloud(ctx, 64)
        handles = (C.c_void_p * LIST)(*[c.h for c in clouds]); one = (C.c_void_p * 1)(empty.h)
        tr = np.ascontiguousarray(np.stack([api._colmajor(T, 4) for T in trs]), F)
        Kp, offp = api._colmajor(proj.cameraMatrix(), 3), api._colmajor(offset, 4)
        app = (C.c_int * LIST)(); fus = (C.c_int * LIST)()

        def call(total, n, h, a_, f_):
            ctx.check(ctx._L.pwn_hip_merge_clouds(ctx.h, api._ptr(Kp), api._ptr(offp), n, h, api._ptr(tr), proj.minDistance(), proj.maxDistance(), rows, cols,
                                                  total.h, api._ptr(weights), a_, f_))
        ms = []
        for rep in range(a.warmup + a.reps):
            total = api.Cloud(ctx, cap)
            call(total, 1, one, None, None)
            ctx.synchronize()
            t = time.perf_counter(); call(total, LIST, handles, app, fus); dt = (time.perf_counter() - t) * 1e3
            if rep >= a.warmup:
                ms.append(dt)
            assert total.size() == sum(app)
            del total

        def mirror():                                              # what PwnMerger.mergeNodeList pays on top: the total and its weights allocated per list
            merger.clearCloud()
            merger.mergeBatch(trs, offset, clouds)
        ms_m = timed(mirror, 1, max(3, a.reps // 4))
        assert list(merger.appended) == list(app) and list(merger.fused) == list(fus)
        points = merger.cloudTot().size()
        appended, fused = list(merger.appended), list(merger.fused)
        sizes = [c.size() for c in clouds]
        before = [0] + list(np.cumsum(appended)[:-1])
        sym6 = clouds[0].omega_storage() == "sym6"
        nbytes = algorithmic_bytes(rows * cols, sizes, [int(b) for b in before], appended, fused, omega_floats=6 if sym6 else 9)
        reps_c = max(3, a.reps // 4)
        res = []
        ms_c = timed(lambda: res.append(composed(ctx, proj, clouds, trs, offset)), 1, reps_c)
        line = dict(bench="merge_clouds", rows=rows, cols=cols, scale=scale, clouds=LIST, reps=a.reps, warmup=a.warmup, source_points=sizes,
                    total_points=points, appended=appended, fused=fused,
                    one_call=dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms)),
                    mirror=dict(ms_median=statistics.median(ms_m), ms_min=min(ms_m), ms_max=max(ms_m)),
                    composed=dict(reps=reps_c, ms_median=statistics.median(ms_c), ms_min=min(ms_c), ms_max=max(ms_c), total_points=res[-1][0],
                                  same_counters=(res[-1][1] == appended and res[-1][2] == fused and res[-1][0] == points)),
                    bytes=nbytes, hbm_read_GBps=read_GBps, hbm_copy_GBps=copy_GBps, floor_ms=nbytes / (read_GBps * 1e9) * 1e3)
        line["one_call_over_floor"] = line["one_call"]["ms_median"] / line["floor_ms"]
        line["composed_over_one_call"] = line["composed"]["ms_median"] / line["one_call"]["ms_median"]
        print(json.dumps(line))
        lines.append(line)
        del merger, clouds
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
