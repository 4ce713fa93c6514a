"""The two host mirrors of the multi-stream tracker held together: api.PwnTrackerBatch (Python) writes its frames, calls, result records, final
states and key clouds to a file, tools/pwn_hip_track_streams_check (PwnTrackerBatch of host/pwn_hip.hpp) runs the same calls and compares result
for result, bit for bit.  The tool exits 0 when nothing differs."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_gives_the_python_mirrors_bits(tmp_path):
    from g2o_frontend_amd import api, synth
    from test_gpu_parity import gpu_objects
    from test_gpu_track_streams import ROWS, COLS, SCALE, THRESHOLD, STREAMS
    S, calls = 3, [1, 4, 3]                      # first frames, a call with key switches, a call with an idle stream
    n = sum(calls)
    K2 = synth.scaled_K(synth.K_VGA, 2)
    Km = np.array([[K2[0], 0, K2[2]], [0, K2[1], K2[3]], [0, 0, 1]], np.float32)
    off = synth.v2t(np.array([0.0, 0.0, 0.0, 0.01, -0.005, 0.0])).astype(np.float32)
    raw = []
    for seed, ts, rs in STREAMS[:S]:
        poses = synth.trajectory(seed, n, ts, rs)
        raw.append([synth.render_depth_mm(seed, poses[k], ROWS, COLS, K2, hole_stream=k) for k in range(n)])
    present = np.ones((n, S), np.int32); present[6, 1] = 0
    ctx = api.Context(0, ROWS, COLS, 4)
    try:
        _, converter, aligner = gpu_objects(ctx, "small")
        tb = api.PwnTrackerBatch(aligner, converter, S, max(calls), ROWS, COLS, SCALE); tb.setNewFrameInliersFraction(THRESHOLD)
        records, f0 = b"", 0
        switches = 0
        for m in calls:
            rows = [[raw[s][f0 + f] if present[f0 + f, s] else None for s in range(S)] for f in range(m)]
            res = tb.processFramesRaw(rows, off, Km)
            records += bytes(res); f0 += m
            switches += sum(int(r.new_frame and r.aligned) for r in res)
        assert switches >= 2
        path = str(tmp_path / "track_streams.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<6i5f", S, n, ROWS, COLS, SCALE, len(calls), float(np.float32(THRESHOLD)), *[float(np.float32(k)) for k in K2]))
            f.write(np.ascontiguousarray(off.T, np.float32).tobytes())
            f.write(np.asarray(calls, np.int32).tobytes()); f.write(present.tobytes())
            for k in range(n):
                for s in range(S):
                    if present[k, s]:
                        f.write(np.ascontiguousarray(raw[s][k], np.uint16).tobytes())
            f.write(records)
            for s in range(S):
                st = tb.state(s)
                pts = tb.keyCloud(s).arrays()["points"]
                f.write(np.ascontiguousarray(st["globalT"].T, np.float32).tobytes()); f.write(np.ascontiguousarray(st["previousCloudTransform"].T, np.float32).tobytes())
                f.write(struct.pack("<3i", st["counter"], st["numKeyframes"], len(pts)))
                f.write(np.ascontiguousarray(pts, np.float32).tobytes())
        del tb
    finally:
        ctx.close()
    exe = os.path.join(ROOT, "tools", "pwn_hip_track_streams_check")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 differences" in r.stdout and "%d key switches" % switches in r.stdout
