"""What tracking S depth streams in lock-step (include/pwn_hip.h: pwn_hip_track_frames, api.PwnTrackerBatch) is worth on one MI355X.

    python tools/bench_track_streams.py [--streams 1,8,32,128] [--frames 1,8] [--scales 2,4] [--rounds 3] [--out profiles/track_streams_bench.jsonl]

VGA frames (480x640, g2o_frontend_amd/synth.py) along four seeded trajectories (stream s follows trajectory s % 4), resident on the device: raw
uint16 for the new call, float metres for api.PwnTracker.  Matcher scale 4 runs the reference's imageScale-4 configuration, scale 2 the VGA
configuration with the Stats radii and point count halved (as the 1280x960 configuration doubles them).  New-frame fraction 0.4 (pwn_tracker.cpp:36).
Per (scale, S, F): every stream takes its first key cloud untimed, then `rounds` rounds; in each round the same F frames per stream go through
  * `batch`: ONE PwnTrackerBatch.processFrames call (F steps of S pairs, one submission, one wait),
  * `single`: S api.PwnTracker objects run one after the other, F processFrame calls each,
  * `prefetch`: the same with nextDepthImage (frame k + 1 converted beside the alignment of frame k),
in the same process, host clock around each; the order of the three rotates from round to round.  The three keep their own states and compute the same poses (`poses_equal_single`: every stream's globalT after every round, all three legs, bit for bit).
One JSON line per (scale, S, F): frames per second of each leg per round and their medians, and the ratio batch / single.
Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from g2o_frontend_amd import conf, synth      # noqa: E402

ROWS, COLS, K = 480, 640, synth.K_VGA
TRAJECTORIES = 4
FRACTION = 0.4


def _render(job):
    seed, k, pose = job
    return synth.render_depth_mm(seed, pose, ROWS, COLS, K, hole_stream=k)


def build_objects(api, ctx, scale):
    cv = dict(conf.QVGA4_CONF_CONVERTER) if scale == 4 else dict(conf.VGA_CONF_CONVERTER, min_image_radius=5, max_image_radius=15, min_points=25)
    al = dict(conf.QVGA4_CONF_ALIGNER) if scale == 4 else dict(conf.VGA_CONF_ALIGNER)
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]); proj.setMinDistance(cv["min_distance"]); proj.setMaxDistance(cv["max_distance"])
    proj.setImageSize(ROWS // scale, COLS // scale)
    st = api.StatsCalculatorIntegralImage()
    st.setWorldRadius(cv["world_radius"]); st.setMinImageRadius(cv["min_image_radius"]); st.setMaxImageRadius(cv["max_image_radius"])
    st.setMinPoints(cv["min_points"]); st.setCurvatureThreshold(cv["stats_curvature_threshold"])
    pi, ni = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
    pi.setCurvatureThreshold(cv["point_info_curvature_threshold"]); ni.setCurvatureThreshold(cv["normal_info_curvature_threshold"])
    converter = api.DepthImageConverterIntegralImage(proj, st, pi, ni)
    f = api.CorrespondenceFinder()
    f.setInlierDistanceThreshold(al["inlier_distance_threshold"]); f.setInlierNormalAngularThreshold(al["inlier_normal_angular_threshold"])
    f.setFlatCurvatureThreshold(al["flat_curvature_threshold"]); f.setInlierCurvatureRatioThreshold(al["inlier_curvature_ratio_threshold"])
    f.setImageSize(ROWS // scale, COLS // scale)
    lin = api.Linearizer(); lin.setInlierMaxChi2(al["inlier_max_chi2"]); lin.setRobustKernel(al["robust_kernel"])
    a = api.Aligner(ctx)
    a.setProjector(proj); a.setLinearizer(lin); a.setCorrespondenceFinder(f)
    a.setOuterIterations(al["outer_iterations"]); a.setInnerIterations(al["inner_iterations"])
    return converter, a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8,32,128")
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--scales", default="2,4")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_streams_bench.jsonl"))
    args = ap.parse_args()
    from g2o_frontend_amd import api
    Ss = [int(x) for x in args.streams.split(",")]; Fs = [int(x) for x in args.frames.split(",")]; scales = [int(x) for x in args.scales.split(",")]
    per_traj = 1 + args.rounds * max(Fs)
    jobs = []
    for t in range(TRAJECTORIES):
        poses = synth.trajectory(11 + t, per_traj)
        jobs += [(11 + t, k, poses[k]) for k in range(per_traj)]
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        rendered = list(ex.map(_render, jobs))
    raw = np.stack(rendered).reshape(TRAJECTORIES, per_traj, ROWS, COLS)
    ctx = api.Context(0, ROWS, COLS, max(Ss))
    I = np.eye(4, dtype=np.float32)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float32)
    draw = api.DeviceBuffer(ctx, raw.reshape(-1, ROWS, COLS))
    dflt = api.DeviceBuffer(ctx, np.where(raw > 0, np.float32(0.001) * raw.astype(np.float32), np.float32(0)).astype(np.float32).reshape(-1, ROWS, COLS))
    u16 = lambda s, k: draw.frame((s % TRAJECTORIES) * per_traj + k)
    f32 = [[dflt.frame(t * per_traj + k) for k in range(per_traj)] for t in range(TRAJECTORIES)]      # the same objects call after call: prefetch() matches by identity
    out = open(args.out, "a")
    for scale in scales:
        converter, aligner = build_objects(api, ctx, scale)
        for S in Ss:
            for F in Fs:
                tb = api.PwnTrackerBatch(aligner, converter, S, F, ROWS, COLS, scale); tb.setNewFrameInliersFraction(FRACTION)
                legs = {}
                for leg in ("single", "prefetch"):
                    legs[leg] = []
                    for s in range(S):
                        tr = api.PwnTracker(aligner, converter); tr.setScale(scale); tr.setNewFrameInliersFraction(FRACTION)
                        legs[leg].append(tr)
                tb.processFrames([[u16(s, 0) for s in range(S)]], I, Km)
                for leg in legs.values():
                    for s, tr in enumerate(leg):
                        tr.processFrame(f32[s % TRAJECTORIES][0], I, Km)
                fps = {"batch": [], "single": [], "prefetch": []}
                switches, equal = 0, True
                for r in range(args.rounds):
                    k0 = 1 + r * F
                    got = {}

                    def run_batch():
                        got["batch"] = [x["globalT"] for x in tb.processFrames([[u16(s, k0 + f) for s in range(S)] for f in range(F)], I, Km)[F - 1]]
                        return got["batch"]

                    def run_single():
                        got["single"] = []
                        for s, tr in enumerate(legs["single"]):
                            for f in range(F):
                                last = tr.processFrame(f32[s % TRAJECTORIES][k0 + f], I, Km)
                            got["single"].append(last["globalT"])

                    def run_prefetch():
                        got["prefetch"] = []
                        for s, tr in enumerate(legs["prefetch"]):
                            fr = f32[s % TRAJECTORIES]
                            for f in range(F):
                                last = tr.processFrame(fr[k0 + f], I, Km, nextDepthImage=fr[k0 + f + 1] if f + 1 < F else None)
                            got["prefetch"].append(last["globalT"])

                    order = [("batch", run_batch), ("single", run_single), ("prefetch", run_prefetch)]
                    order = order[r % 3:] + order[:r % 3]                      # the legs alternate: each is first, second and third once in three rounds
                    for name, fn in order:
                        t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
                        fps[name].append(S * F / dt)
                    for s in range(S):                                        # every stream's pose after the round, all three legs, bit for bit
                        equal = equal and all(np.array_equal(got["batch"][s].view(np.uint32), got[leg][s].view(np.uint32)) for leg in ("single", "prefetch"))
                    switches += sum(int(tb.numKeyframes(s)) for s in range(S)) if r == args.rounds - 1 else 0
                med = {k: statistics.median(v) for k, v in fps.items()}
                line = dict(bench="track_streams", rows=ROWS, cols=COLS, scale=scale, streams=S, frames_per_call=F, rounds=args.rounds, keyframes=switches, poses_equal_single=bool(equal),
                            frames_per_s={k: [round(x, 1) for x in v] for k, v in fps.items()}, median_frames_per_s={k: round(v, 1) for k, v in med.items()},
                            batch_over_single=round(med["batch"] / med["single"], 2), batch_over_prefetch=round(med["batch"] / med["prefetch"], 2),
                            ms_per_frame_batch=round(1e3 / med["batch"], 4))
                print(json.dumps(line)); out.write(json.dumps(line) + "\n"); out.flush()
                del tb, legs
    out.close()
    ctx.close()


if __name__ == "__main__":
    main()
