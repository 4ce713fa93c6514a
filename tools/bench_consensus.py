"""What the consensus validation of a partition's closures costs: the device call (include/pwn_hip.h: pwn_hip_validate_relations) against the same
text run serially on the box's host (pwn_hip_validate_relations_host).

    python tools/bench_consensus.py [--sizes 128 1024 4096] [--reps 5] [--out profiles/consensus_bench.jsonl]

Per size n: n relations of the drift scenario (two partitions of 5 and 7 key nodes, 30 % gross outliers, consistent orientation), built by the
generator below.  The device call takes the transforms from closure records resident on the device ([n, 128] float32), the poses, flags and
counters from host arrays (uploaded inside the call) and returns counters and decisions to host arrays; the error matrices are not requested on
either side.  Host clock around each call (the device call ends in the library's one wait), both in this process, alternating, --reps repeats
after one warm-up each; median, minimum and maximum.  The two calls see the same float-rounded transforms, so their counters and decisions are
compared as well (`equal`).  The stage times come from one profiled device call.  One JSON line per size.  Needs a GPU."""
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

from g2o_frontend_amd import _lib, api      # noqa: E402

STAGES = ("consensus_prepare", "consensus_errors", "consensus_count", "consensus_commit")


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _iso(R, t):
    X = np.eye(4); X[:3, :3] = R; X[:3, 3] = t
    return X


def scenario(n, seed=0, outliers=0.3):
    """-> tc, to [n, 16] float64 column-major, records [n, 128] float32 (T = words [0:16]), flags (all set: the consistent orientation), good"""
    rng = np.random.default_rng(seed)
    cur = [_iso(_rotation((0, 0, 1), rng.uniform(-1.2, 1.2)), (rng.uniform(-3, 3), rng.uniform(-3, 3), 0.0)) for _ in range(5)]
    oth = [_iso(_rotation((0, 0, 1), 2.5 + rng.uniform(-1.2, 1.2)), (rng.uniform(-3, 3), 2.0 + rng.uniform(-3, 3), 0.0)) for _ in range(7)]
    D = _iso(_rotation((0.1, -0.2, 1.0), np.deg2rad(20.0)), (1.5, -0.8, 0.3))
    good = np.ones(n, bool); good[rng.permutation(n)[:int(round(outliers * n))]] = False
    tc, to, tr = [], [], []
    for k in range(n):
        a, b = int(rng.integers(5)), int(rng.integers(7))
        tc.append(cur[a]); to.append(D @ oth[b])
        if good[k]:
            tr.append(np.linalg.inv(cur[a]) @ oth[b] @ _iso(_rotation(rng.normal(size=3), rng.normal() * 3e-3), rng.normal(size=3) * 1e-2))
        else:
            tr.append(_iso(_rotation(rng.normal(size=3), rng.uniform(0, np.pi)), rng.uniform(-3, 3, 3)))
    cm = lambda Ts: np.ascontiguousarray(np.stack(Ts).transpose(0, 2, 1).reshape(n, 16))
    records = np.zeros((n, 128), np.float32); records[:, :16] = cm(tr).astype(np.float32)
    return cm(tc), cm(to), records, np.ones(n, np.int32), good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 1024, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_bench.jsonl"))
    args = ap.parse_args()
    L = _lib.lib()
    ctx = api.Context(device=0, max_rows=120, max_cols=160, max_batch=1)
    p = _lib.ConsensusParams(); L.pwn_hip_default_consensus_params(C.byref(p)); p.min_times_checked = 1
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lines = []
    for n in args.sizes:
        tc, to, records, flags, good = scenario(n, seed=n)
        rec_dev = api.DeviceBuffer(ctx, records)
        tr_host = np.ascontiguousarray(records[:, :16].astype(np.float64))          # what the device reads of the records
        tr_host[:, [3, 7, 11]] = 0.0; tr_host[:, 15] = 1.0

        def device():
            cnt = [np.zeros(n, np.int32) for _ in range(3)]; dec = np.zeros(n, np.int32)
            t = time.perf_counter()
            ctx.check(L.pwn_hip_validate_relations(ctx.h, C.byref(p), n, vp(tc), vp(to), None, C.c_void_p(rec_dev.data_ptr()), 128, vp(flags), vp(cnt[0]), vp(cnt[1]),
                                                   vp(cnt[2]), vp(dec), None, None))
            return (time.perf_counter() - t) * 1e3, cnt, dec

        def host():
            cnt = [np.zeros(n, np.int32) for _ in range(3)]; dec = np.zeros(n, np.int32)
            t = time.perf_counter()
            rc = L.pwn_hip_validate_relations_host(C.byref(p), n, vp(tc), vp(to), vp(tr_host), vp(flags), vp(cnt[0]), vp(cnt[1]), vp(cnt[2]), vp(dec), None, None, None)
            assert rc == 0, L.pwn_hip_last_error_string(None)
            return (time.perf_counter() - t) * 1e3, cnt, dec

        device(); host()                                                             # warm-up: the scratch grows, the pages are touched
        td, th = [], []
        for _ in range(args.reps):
            ms, dcnt, ddec = device(); td.append(ms)
            ms, hcnt, hdec = host(); th.append(ms)
        ctx.check(L.pwn_hip_set_profiling(ctx.h, 1))
        device()
        stages = {s: round(ctx.stage_ms(s)[0], 4) for s in STAGES}
        ctx.check(L.pwn_hip_set_profiling(ctx.h, 0))
        line = {"bench": "consensus", "relations": n, "pair_evaluations": n * n, "reps": args.reps,
                "device_ms": round(statistics.median(td), 4), "device_min_max_ms": [round(min(td), 4), round(max(td), 4)],
                "host_ms": round(statistics.median(th), 4), "host_min_max_ms": [round(min(th), 4), round(max(th), 4)],
                "host_over_device": round(statistics.median(th) / statistics.median(td), 2), "device_stage_ms": stages,
                "equal": bool(all(np.array_equal(a, b) for a, b in zip(dcnt + [ddec], hcnt + [hdec]))),
                "accepted": int((ddec == 1).sum()), "good": int(good.sum()), "accepted_are_the_good": bool(np.array_equal(ddec == 1, good))}
        print(json.dumps(line), flush=True)
        lines.append(line)
    ctx.close()
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
