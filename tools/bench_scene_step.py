#!/usr/bin/env python3
"""The mapping loop (pwn_aligner.cpp:166-209) per frame on one MI355X: the composed route -- pwn_hip_convert_batch_ex, pwn_hip_project into a device
image, pwn_hip_convert_batch, pwn_hip_align, pwn_hip_iso_mul, pwn_hip_cloud_add, pwn_hip_merge -- against pwn_hip_scene_step.

    python tools/bench_scene_step.py [--frames 30] [--parent-lib PATH] [--out profiles/scene_step_bench.jsonl]

VGA room frames (uint16 millimetres, resident on the device), one chunk of --frames frames, at step 1 (the frame as it is) and step 2
(DepthImage_scale in front: 240x320 clouds).  The two routes alternate frame about within one process, on twin scenes that hold the same bytes;
which route goes first alternates too.  Host clock around a frame, median over frames 5 .. frames - 1.  With --parent-lib the composed route is
timed once more on THAT library (the parent commit's build) in a child process of the same session.  Per step one JSON line: the medians, the
per-stage device times of the one-call route from a second, profiled pass (event timing adds host time, so it is kept out of the timed pass),
and whether the two routes ended on the same scene size.  Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_STAGES = ("scene_render", "scene_pose", "scene_add", "scene_merge")
STAGES = ("depth_scale", "unproject", "integral_rows", "integral_cols", "stats", "gaussians", "project_cur", "project_ref", "corr_linearize", "solve") + NEW_STAGES


def frames_mm(n):
    from g2o_frontend_amd import synth
    poses = synth.trajectory(5, n)
    return [synth.render_depth_mm(5, poses[k], 480, 640, synth.K_VGA, hole_stream=k) for k in range(n)]


class Rig:
    def __init__(self, ctx, step, n, one_call):
        import bench
        from g2o_frontend_amd import api
        self.ctx, self.step = ctx, step
        self.rows, self.cols = (480 // step, 640 // step)
        K, conv, alig = bench.conf(self.rows, self.cols)
        self.converter, self.aligner = bench.build_objects(ctx, self.rows, self.cols, K, conv, alig)
        self.proj = self.converter.projector()
        self.merger = api.Merger(); self.merger.setDepthImageConverter(self.converter); self.merger.setImageSize(self.rows, self.cols)
        self.cp, self.ap = self.converter.params(None), self.aligner.params()
        pixels = self.rows * self.cols
        self.scene, self.cloud, self.sub = api.Cloud(ctx, (n + 1) * pixels), api.Cloud(ctx, pixels), api.Cloud(ctx, pixels)
        self.sceneT = np.eye(4, dtype=np.float32)
        self.image = api.DeviceBuffer(ctx, np.zeros((self.rows, self.cols), np.float32))
        self.K = api._colmajor(self.proj.cameraMatrix(), 3)
        self.I = np.eye(4, dtype=np.float32)
        if one_call:
            self.sp = api.SceneStepParams()
            ctx._L.pwn_hip_default_scene_step_params(C.byref(self.sp))
            self.sp.normal_threshold = self.merger.normalThreshold()
            self.sp.step = 0 if step == 1 else step

    def _mul(self, A, B):
        from g2o_frontend_amd.api import _colmajor, _from_colmajor, _ptr
        out = np.empty(16, np.float32)
        self.ctx._L.pwn_hip_iso_mul(_ptr(_colmajor(A, 4)), _ptr(_colmajor(B, 4)), _ptr(out))
        return _from_colmajor(out, 4)

    def composed(self, frame):
        from g2o_frontend_amd import api
        from g2o_frontend_amd.api import _colmajor, _ptr
        ctx, L, m = self.ctx, self.ctx._L, self.merger
        ex = api.ConvertExtras(1, 1, self.proj.baseline(), self.proj.alpha())
        ctx.check(L.pwn_hip_convert_batch_ex(ctx.h, C.byref(self.cp), (C.c_void_p * 1)(_ptr(frame)), 1, 0.001, 1, 480, 640, 0 if self.step == 1 else self.step, 0.01,
                                             C.byref(ex), (C.c_void_p * 1)(self.cloud.h)))
        ctx.check(L.pwn_hip_project(ctx.h, _ptr(self.K), _ptr(_colmajor(self._mul(self.sceneT, self.I), 4)), self.proj.minDistance(), self.proj.maxDistance(),
                                    self.rows, self.cols, self.scene.h, None, _ptr(self.image)))
        ctx.check(L.pwn_hip_convert_batch(ctx.h, C.byref(self.cp), (C.c_void_p * 1)(_ptr(self.image)), 1, self.rows, self.cols, (C.c_void_p * 1)(self.sub.h)))
        res = api.AlignResult()
        ctx.check(L.pwn_hip_align(ctx.h, C.byref(self.ap), self.sub.h, self.cloud.h, C.byref(res)))
        self.sceneT = self._mul(self.sceneT, api._from_colmajor(res.T, 4)); self.sceneT[3] = (0, 0, 0, 1)
        ctx.check(L.pwn_hip_cloud_add(ctx.h, self.scene.h, self.cloud.h, _ptr(_colmajor(self.sceneT, 4))))
        k = C.c_int(0)
        ctx.check(L.pwn_hip_merge(ctx.h, self.scene.h, _ptr(self.K), _ptr(_colmajor(self._mul(self.sceneT, self.I), 4)), self.proj.minDistance(), self.proj.maxDistance(),
                                  self.rows, self.cols, m.distanceThreshold(), m.normalThreshold(), m.maxPointDepth(), C.byref(k), None))
        return k.value

    def one_call(self, frame):
        from g2o_frontend_amd import api
        res = api.scene_step(self.ctx, self.cp, self.ap, self.sp, frame, self.sceneT, self.scene, self.cloud, self.sub, raw_scale=0.001)
        self.sceneT = api._from_colmajor(res.scene_T, 4)
        return res.size_after_merge


def run(step, frames, composed_only):
    from g2o_frontend_amd import api
    ctx = api.Context(0, 480, 640, 2)
    dev = [api.DeviceBuffer(ctx, f) for f in frames]
    n = len(frames)
    a, b = Rig(ctx, step, n, False), (None if composed_only else Rig(ctx, step, n, True))
    t = {"composed": [], "one_call": []}
    sizes = {"composed": 0, "one_call": 0}
    for k, f in enumerate(dev):
        order = ("composed", "one_call") if k % 2 == 0 else ("one_call", "composed")
        for route in order:
            rig = a if route == "composed" else b
            if rig is None:
                continue
            t0 = time.perf_counter()
            sizes[route] = rig.composed(f) if route == "composed" else rig.one_call(f)
            t[route].append((time.perf_counter() - t0) * 1e3)
    line = dict(step=step, frames=n, composed_ms=round(float(np.median(t["composed"][5:])), 4), composed_scene_points=sizes["composed"])
    if b is not None:
        line.update(one_call_ms=round(float(np.median(t["one_call"][5:])), 4), one_call_scene_points=sizes["one_call"], same_scene_size=sizes["composed"] == sizes["one_call"])
        line["composed_over_one_call"] = round(line["composed_ms"] / line["one_call_ms"], 3)
        # the stages of the one-call route: a second pass over the chunk on a fresh scene, profiled
        ctx.set_profiling(True)
        p = Rig(ctx, step, n, True)
        acc = {s: [] for s in STAGES}
        for k, f in enumerate(dev):
            p.one_call(f)
            if k >= 5:
                for s in STAGES:
                    acc[s].append(ctx.stage_ms(s)[0])
        ctx.set_profiling(False)
        line["one_call_stage_ms"] = {s: round(float(np.median(v)), 4) for s, v in acc.items() if v and max(v) > 0}
    ctx.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--parent-lib", default=None, help="libpwn_hip.so built from the parent commit: the composed route is timed on it in a child process")
    ap.add_argument("--composed-only", action="store_true", help="(the child) only the composed route: the library may lack pwn_hip_scene_step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.composed_only:
        from g2o_frontend_amd import _lib
        for name in ("pwn_hip_scene_step", "pwn_hip_default_scene_step_params"):
            _lib.PROTOTYPES.pop(name, None)
    frames = frames_mm(args.frames)
    lines = [run(step, frames, args.composed_only) for step in (1, 2)]
    if args.parent_lib and not args.composed_only:
        env = dict(os.environ, PWN_HIP_LIB=os.path.abspath(args.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--frames", str(args.frames), "--composed-only"], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("child on the parent library failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        child = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
        for ln, ch in zip(lines, child):
            ln["parent_library_composed_ms"] = ch["composed_ms"]
            ln["parent_library_scene_points"] = ch["composed_scene_points"]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
