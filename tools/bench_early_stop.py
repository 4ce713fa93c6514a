"""What "stop when converged" (include/pwn_hip.h: pwn_hip_ctx_set_convergence) is worth on one MI355X.

    python tools/bench_early_stop.py [--pairs 128] [--reps 10] [--warmup 3] [--out profiles/early_stop_bench.jsonl]

128 seeded VGA pairs (g2o_frontend_amd/synth.py), default sym6 clouds, the reference's VGA configuration with ten outer iterations, two workloads:
  * `match_batch_records`: the loop-closure call on resident clouds -- pwn_hip_match_batch_records with the closer's kind of guess (the true pose
    off by <= 1 cm / 0.5 deg per axis, z translation zeroed, pwn_matcher_base.cpp:114), scores and 72-word records;
  * `fused_step`: pwn_hip_convert_align_batch_u16 from device-resident uint16 frames, identity guesses, 64-word records.
Three settings: off, (1e-3 m, 1e-4) and (1e-4 m, 1e-5), both with min_iterations 2.  After a warm-up the settings are timed alternately in the same
process (off, a, b, off, a, b, ...), host clock around calls that end in the library's wait for the device.  One JSON line per workload and setting:
  * pairs_per_s from the median call, with the fastest and the slowest call;
  * the histogram and the mean of the executed outer iterations (pwn_hip_last_align_steps);
  * the largest distance of a pair's final pose from its ten-iteration pose: translation and rotation norms of t2v(inv(T_10) T), float64;
  * for the closure call, the PwnCloserAcceptance decisions that differ from the ten-iteration run's;
  * predicted_ms: the off run's median scaled by the loop's share of its per-stage timers (project_ref + corr_linearize + solve of all, from one
    profiled call) times the executed share of iterations -- what the call would take if a skipped iteration cost nothing -- beside the measured
    saving; `off_spread_ms` is the off runs' own max - min.
Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
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
OUTER = 10
SETTINGS = (("off", None), ("1e-3/1e-4", (1e-3, 1e-4, 2)), ("1e-4/1e-5", (1e-4, 1e-5, 2)))
LOOP_STAGES = ("project_ref", "corr_linearize", "solve")
ALL_STAGES = ("unproject", "integral", "integral_rows", "integral_cols", "stats", "project_cur", "match_score") + LOOP_STAGES


def _render(seed):
    return synth.make_pair(seed, ROWS, COLS, K)[:2]


def closure_guesses(seeds, t_noise=0.01, q_noise=0.004):
    g = np.empty((len(seeds), 16), np.float32)
    for i, s in enumerate(seeds):
        u = synth._uniform(s, 7, 6)
        dv = np.concatenate([(2 * u[0:3] - 1) * t_noise, (2 * u[3:6] - 1) * q_noise])
        T = (synth.pair_pose(s) @ synth.v2t(dv)).astype(np.float32)
        T[2, 3] = 0.0; T[3] = (0, 0, 0, 1)
        g[i] = T.T.reshape(-1)
    return g


def build_objects(api, ctx):
    cv, al = conf.VGA_CONF_CONVERTER, conf.VGA_CONF_ALIGNER
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]); proj.setMinDistance(cv["min_distance"]); proj.setMaxDistance(cv["max_distance"])
    proj.setImageSize(ROWS, COLS)
    st = api.StatsCalculatorIntegralImage()
    st.setWorldRadius(cv["world_radius"]); st.setMinImageRadius(cv["min_image_radius"]); st.setMaxImageRadius(cv["max_image_radius"])
    st.setMinPoints(cv["min_points"]); st.setCurvatureThreshold(cv["stats_curvature_threshold"])
    pi, ni = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
    pi.setCurvatureThreshold(cv["point_info_curvature_threshold"]); ni.setCurvatureThreshold(cv["normal_info_curvature_threshold"])
    converter = api.DepthImageConverterIntegralImage(proj, st, pi, ni)
    f = api.CorrespondenceFinder()
    f.setInlierDistanceThreshold(al["inlier_distance_threshold"]); f.setInlierNormalAngularThreshold(al["inlier_normal_angular_threshold"])
    f.setFlatCurvatureThreshold(al["flat_curvature_threshold"]); f.setInlierCurvatureRatioThreshold(al["inlier_curvature_ratio_threshold"])
    f.setImageSize(ROWS, COLS)
    lin = api.Linearizer(); lin.setInlierMaxChi2(al["inlier_max_chi2"]); lin.setRobustKernel(al["robust_kernel"])
    a = api.Aligner(ctx)
    a.setProjector(proj); a.setLinearizer(lin); a.setCorrespondenceFinder(f)
    a.setOuterIterations(OUTER); a.setInnerIterations(1)
    return converter, a


def pose_distance(T, T10):
    """(translation, rotation) norms of t2v(inv(T10) T), float64; T: column-major 16 floats"""
    A = np.asarray(T, np.float64).reshape(4, 4).T; B = np.asarray(T10, np.float64).reshape(4, 4).T
    Bi = np.eye(4); Bi[:3, :3] = B[:3, :3].T; Bi[:3, 3] = -B[:3, :3].T @ B[:3, 3]
    M = Bi @ A
    R = M[:3, :3]
    qw = 0.5 * np.sqrt(max(0.0, 1.0 + np.trace(R)))
    q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4.0 * qw)
    return float(np.linalg.norm(M[:3, 3])), float(np.linalg.norm(q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.pairs
    seeds = list(range(n))
    with ProcessPoolExecutor(min(16, n)) as ex:                      # before the device is opened: the workers only render
        frames = list(ex.map(_render, seeds))
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import AlignResult, MatchResult
    ctx = api.Context(0, ROWS, COLS, max(n, 1))
    L = ctx._L
    converter, aligner = build_objects(api, ctx)
    refs = [api.Cloud(ctx, ROWS * COLS) for _ in range(n)]; curs = [api.Cloud(ctx, ROWS * COLS) for _ in range(n)]
    dev = [ctx.upload(f) for pair in frames for f in pair]
    rf, cf = dev[0::2], dev[1::2]
    converter.computeBatch(refs + curs, rf + cf, raw_scale=0.001)
    p = aligner.params()
    hr = (C.c_void_p * n)(*[c.h for c in refs]); hc = (C.c_void_p * n)(*[c.h for c in curs])
    g = closure_guesses(seeds); gp = g.ctypes.data_as(C.c_void_p)
    res = (AlignResult * n)(); scores = (MatchResult * n)()
    rec72 = ctx.upload(np.zeros((n, api.MATCH_RECORD_FLOATS), np.float32)); rec64 = ctx.upload(np.zeros((n, api.RECORD_FLOATS), np.float32))
    prepared = aligner.convertAlignHandles(refs, curs, rf, cf, converter=converter)
    acc = api.PwnCloserAcceptance()

    def match():
        ctx.check(L.pwn_hip_match_batch_records(ctx.h, C.byref(p), n, hr, hc, gp, 50.0, None, 0, res, scores, C.c_void_p(rec72.data_ptr())))
        return np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=n)

    def fused():
        return aligner.convertAlignBatch(converter, None, None, None, None, raw_scale=0.001, records=rec64, prepared=prepared)

    def accepted():
        return [acc.accept(dict(image_nonZeros=m.image_non_zeros, image_outliers=m.image_outliers, image_inliers=m.image_inliers)) for m in scores]

    def set_(setting):
        if setting is None:
            ctx.clear_convergence()
        else:
            ctx.set_convergence(*setting)

    lines = []
    for wname, call in (("match_batch_records", match), ("fused_step", fused)):
        # ten-iteration reference, the loop's share of the stage timers (one profiled call), warm-up of every setting
        set_(None)
        r10 = call().copy(); acc10 = accepted() if call is match else None
        ctx.set_profiling(True); call(); stage = {k: ctx.stage_ms(k)[0] for k in ALL_STAGES}; ctx.set_profiling(False)
        loop_share = sum(stage[k] for k in LOOP_STAGES) / max(sum(stage.values()), 1e-9)
        info = {}
        for sname, setting in SETTINGS:
            set_(setting)
            for _ in range(args.warmup):
                r = call()
            steps = ctx.last_align_steps(0, n)
            its = [s["iterations"] for s in steps]
            d = [pose_distance(r["T"][i], r10["T"][i]) for i in range(n)]
            info[sname] = dict(hist={str(k): its.count(k) for k in sorted(set(its))}, mean=float(np.mean(its)), converged=sum(1 for s in steps if s["converged"]),
                               dt=max(x[0] for x in d), dr=max(x[1] for x in d),
                               flips=(sum(1 for a, b in zip(accepted(), acc10) if a != b) if call is match else None))
        times = {sname: [] for sname, _ in SETTINGS}
        for _ in range(args.reps):
            for sname, setting in SETTINGS:
                set_(setting)
                t0 = time.perf_counter(); call(); times[sname].append((time.perf_counter() - t0) * 1e3)
        set_(None)
        off = statistics.median(times["off"]); spread = max(times["off"]) - min(times["off"])
        for sname, setting in SETTINGS:
            t = times[sname]; med = statistics.median(t); i = info[sname]
            predicted = off * (1.0 - loop_share * (1.0 - i["mean"] / OUTER))
            lines.append(dict(workload=wname, pairs=n, rows=ROWS, cols=COLS, omega_storage=ctx.omega_storage, outer_iterations=OUTER, setting=sname,
                              translation_epsilon=None if setting is None else setting[0], rotation_epsilon=None if setting is None else setting[1],
                              min_iterations=None if setting is None else setting[2],
                              call_ms=round(med, 3), call_min_max_ms=[round(min(t), 3), round(max(t), 3)], pairs_per_s=round(n / med * 1e3, 1),
                              executed_iterations_histogram=i["hist"], executed_iterations_mean=round(i["mean"], 3), pairs_converged=i["converged"],
                              max_translation_from_ten_iterations_m=i["dt"], max_rotation_from_ten_iterations=i["dr"],
                              closer_acceptance_decisions_changed=i["flips"],
                              off_ms=round(off, 3), off_spread_ms=round(spread, 3), loop_share_of_stage_timers=round(loop_share, 3),
                              predicted_ms=round(predicted, 3), predicted_saving_ms=round(off - predicted, 3), measured_saving_ms=round(off - med, 3),
                              stage_ms_off={k: round(v, 3) for k, v in stage.items() if v}))
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
