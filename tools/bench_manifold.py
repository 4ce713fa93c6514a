"""Timing of the traversability image (ManifoldVoronoiExtractor::process, pwn_tracker2) on one MI355X.

    python tools/bench_manifold.py [--reps 20] [--warmup 3] [--seed 3] [--out profiles/manifold_bench.jsonl]

The deque of 30 key clouds (dequeSize's default) of seeded VGA room frames (g2o_frontend_amd/synth.py) under a sensor mounting with z up, matcher
at scale 2 (240 x 320 clouds) and at scale 1 (480 x 640), splatted into 100 x 100 cells of 0.2 m in the frame of the last node.  Per scale, one
JSON line:
  * `one_call`: pwn_hip_manifold_image of the 30 resident clouds into a host image -- host clock around the call, which ends in its one wait
    for the device; median, minimum and maximum over the repetitions; `device_image`: the same into device memory;
  * `composed`, for information: the same image from the calls that existed before -- Cloud.add of every cloud into a scratch cloud for the
    transformed arrays, its download, the splat in numpy (events sorted by cell, a segmented running minimum: no point here is above 10 m or
    below -55 m, so no height wraps).  Its image is checked against the one call's;
  * `events` (points inside the grid whose normal passes), `largest_run` (events of the fullest cell), `bytes`: what the kernels of the one
    call have to move, computed from the shapes (algorithmic_bytes), and `floor_ms`: those bytes over the streaming-read rate this GPU
    delivered in the same process (pwn_hip_measure_hbm).  one_call / floor says how far the call is from its traffic.
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

from g2o_frontend_amd import api, synth      # noqa: E402
from tools.bench_merge_clouds import build_objects, timed      # noqa: E402

ROWS, COLS, K = 480, 640, synth.K_VGA
DEQUE = 30
XS = YS = 100
RESOLUTION, THRESHOLD = 0.2, 0.64
F = np.float32
OFFSET = np.array([[0, 0, 1, 0.1], [-1, 0, 0, 0.02], [0, -1, 0, 0.3], [0, 0, 0, 1]], F)      # camera looking along the robot's x, z up


def algorithmic_bytes(points, cells):
    """bytes of one pwn_hip_manifold_image call: per point xyz and normal read (28) and key + height written (12); per radix pass the keys read
    for the histogram (8) and keys + heights read and written by the scatter (24); the keys read for the run starts (8) and keys + heights
    read by the cell walk (at most 12); per cell the start word written twice and read, the image read and written"""
    bits = int(cells).bit_length()
    passes = (bits + 7) // 8
    return points * (28 + 12 + 32 * passes + 8 + 12) + cells * (12 + 4)


def numpy_splat(P, N, order_base=None):
    """the image of concatenated transformed points / normals (in list order) in numpy -> (image, events, largest run)"""
    cx, cy, ires = int(XS * 0.5), int(YS * 0.5), F(1.0 / float(F(RESOLUTION)))
    x = np.trunc(F(cx) + P[:, 0] * ires).astype(np.int64); y = np.trunc(F(cy) + P[:, 1] * ires).astype(np.int64)
    pz = np.trunc(F(10000) - F(1000) * P[:, 2]).astype(np.int64)
    sq = ((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]).astype(np.float64)
    keep = (x >= 0) & (x < XS) & (y >= 0) & (y < YS) & ~(sq < 0.1)
    cell, pz, bad = (x * YS + y)[keep], pz[keep], (N[:, 2] < F(THRESHOLD))[keep]
    assert ((pz >= 0) & (pz < 65535)).all(), "a wrapped height: the running minimum does not model it"
    perm = np.argsort(cell, kind="stable")
    cell, pz, bad = cell[perm], pz[perm], bad[perm]
    big = 1 << 17
    good = np.where(bad, 30000, np.minimum(pz, 30000))
    run = np.maximum.accumulate(cell * big + (big - 1 - good))                 # per cell: the lowest stored height up to and including the event
    first = np.r_[True, cell[1:] != cell[:-1]]
    before = np.where(first, 30000, big - 1 - (np.r_[0, run[:-1]] - cell * big))
    hit = bad & (pz <= before)                                                  # a bad point not above the height so far: the cell is an obstacle
    img = np.full(XS * YS, 30000, np.int64)
    last = np.r_[cell[1:] != cell[:-1], True]
    img[cell[last]] = big - 1 - (run[last] - cell[last] * big)
    img[np.unique(cell[hit])] = 65535
    starts = np.nonzero(first)[0]
    return img.reshape(XS, YS).astype(np.uint16), int(len(cell)), int(np.diff(np.r_[starts, len(cell)]).max()) if len(cell) else 0


def composed(ctx, clouds, transforms):
    P, N = [], []
    for c, T in zip(clouds, transforms):
        scratch = api.Cloud(ctx, max(1, c.size()))
        scratch.add(c, T)
        a = scratch.arrays()
        P.append(a["points"][:, :3]); N.append(a["normals"][:, :3])
    return numpy_splat(np.concatenate(P), np.concatenate(N))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("bench_manifold: no HIP device (there is no CPU fallback)")
    ctx = api.Context(device=0, max_rows=ROWS, max_cols=COLS, max_batch=DEQUE)
    read_GBps, copy_GBps = ctx.measure_hbm()
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], F)
    cam = synth.trajectory(a.seed, DEQUE, t_step=0.08, r_step_deg=4.0)
    frames = [synth.render_depth_mm(a.seed, cam[k], ROWS, COLS, K, hole_stream=k).astype(F) * F(0.001) for k in range(DEQUE)]
    poses = [np.asarray(c, np.float64) @ np.linalg.inv(OFFSET.astype(np.float64)) for c in cam]
    nodes = [api.MapNode(k, poses[k], OFFSET) for k in range(DEQUE)]
    trs = [api.ManifoldVoronoiExtractor.nodeTransform(nodes[-1], o) for o in nodes]
    tr = np.ascontiguousarray(np.stack([api._colmajor(T, 4) for T in trs]), F)
    lines = []
    for scale in (2, 1):
        proj, converter, matcher = build_objects(ctx, scale)
        clouds = matcher.makeCloudBatch(Km, OFFSET, frames)[0]
        handles = (C.c_void_p * DEQUE)(*[c.h for c in clouds])
        inside = (C.c_int * DEQUE)()
        host = np.zeros((XS, YS), np.uint16)
        dev = api.DeviceBuffer(ctx, host)

        def call(image):
            ctx.check(ctx._L.pwn_hip_manifold_image(ctx.h, DEQUE, handles, api._ptr(tr), RESOLUTION, XS, YS, THRESHOLD, 0, api._ptr(image), inside))
        ms = timed(lambda: call(host), a.warmup, a.reps)
        ms_d = timed(lambda: call(dev), a.warmup, a.reps)
        assert np.array_equal(dev.numpy(), host)
        reps_c = max(2, a.reps // 10)
        res = []
        ms_c = timed(lambda: res.append(composed(ctx, clouds, trs)), 1, reps_c)
        img_c, events, largest = res[-1]
        sizes = [c.size() for c in clouds]
        points = sum(sizes)
        nbytes = algorithmic_bytes(points, XS * YS)
        line = dict(bench="manifold_image", rows=proj.imageRows(), cols=proj.imageCols(), scale=scale, clouds=DEQUE, grid=[XS, YS], resolution=RESOLUTION,
                    reps=a.reps, warmup=a.warmup, points=points, inside=sum(inside), events=events, largest_run=largest,
                    obstacle_cells=int((host == 65535).sum()), height_cells=int(((host != 65535) & (host != 30000)).sum()),
                    one_call=dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms)),
                    device_image=dict(ms_median=statistics.median(ms_d), ms_min=min(ms_d), ms_max=max(ms_d)),
                    composed=dict(reps=reps_c, ms_median=statistics.median(ms_c), ms_min=min(ms_c), ms_max=max(ms_c), same_image=bool(np.array_equal(img_c, host))),
                    bytes=nbytes, hbm_read_GBps=read_GBps, hbm_copy_GBps=copy_GBps, floor_ms=nbytes / (read_GBps * 1e9) * 1e3)
        line["one_call_over_floor"] = line["one_call"]["ms_median"] / line["floor_ms"]
        line["composed_over_one_call"] = line["composed"]["ms_median"] / line["one_call"]["ms_median"]
        print(json.dumps(line))
        lines.append(line)
        del clouds
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
