"""The mapping step through the C++ host mirror: tools/pwn_hip_scene_step_check (SceneAligner of pwn_hip.hpp against the Python mirror's
results for the same frames) and tools/pwn_hip_scene_aligner --one-call against its default, composed run on the same list."""
import os
import struct
import subprocess

import numpy as np
import pytest

import scene_stream as S
from conftest import case_params
from test_cpp_harness import write_pgm16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CONF = """// pwn_core/conf/pwn_aligner_1_4.conf values for frames of twice the converted size
depthScale 0.001
imageScale 2
fx 262.5
fy 262.5
cx 159.75
cy 119.75
minDistance 0.5
maxDistance 4.5
minImageRadius 3
maxImageRadius 6
minPoints 10
curvatureThreshold 0.2
worldRadius 0.1
informationMatrixCurvatureThreshold 0.02
inlierDistanceThreshold 0.5
inlierNormalAngularThreshold 0.95
inlierCurvatureRatioThreshold 1.3
flatCurvatureThreshold 0.02
inlierMaxChi2 9000
robustKernel 1
outerIterations 10
innerIterations 1
chunkStep 3
"""


def test_cpp_scene_aligner_equals_the_python_mirror(tmp_path, oracle):
    from g2o_frontend_amd import api, build
    from test_gpu_parity import gpu_objects
    build.build_tools()
    rows, cols, K, conv, alig = case_params(S.NAME)
    frames = S.stream_s(oracle)
    ctx = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=2)
    try:
        _, converter, aligner = gpu_objects(ctx, S.NAME)
        merger = api.Merger(); merger.setDepthImageConverter(converter); merger.setImageSize(rows, cols)
        sa = api.SceneAligner(ctx, converter, aligner, merger, (len(frames) + 1) * rows * cols)
        per_frame = b""
        for f in frames:
            T = sa.processFrame(f)
            per_frame += b"".join(np.ascontiguousarray(M.T, np.float32).tobytes() for M in (T, sa.sceneT(), sa.globalT()))
            per_frame += struct.pack("<4i", *sa._sizes)
        scene = sa.scene()
        a = scene.arrays(stats=True)
        path = str(tmp_path / "step.bin")
        with open(path, "wb") as out:
            out.write(struct.pack("<3i", rows, cols, len(frames)))
            out.write(struct.pack("<7d", *K, conv["min_distance"], conv["max_distance"], alig["inlier_distance_threshold"]))
            out.write(struct.pack("<3i", conv["min_image_radius"], conv["max_image_radius"], conv["min_points"]))
            for f in frames:
                out.write(np.ascontiguousarray(f, np.float32).tobytes())
            out.write(per_frame)
            out.write(struct.pack("<2i", scene.size(), scene.numGaussians()))
            for k in ("points", "normals", "curvature", "omega_p", "omega_n", "stats"):
                b = a[k].tobytes()
                out.write(struct.pack("<q", len(b))); out.write(b)
        r = subprocess.run([os.path.join(ROOT, "tools", "pwn_hip_scene_step_check"), path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert " 0 differences" in r.stdout
    finally:
        ctx.close()


def test_scene_aligner_tool_one_call_writes_the_same_trajectory(tmp_path):
    from g2o_frontend_amd import build
    build.build_tools()
    exe = os.path.join(ROOT, "tools", "pwn_hip_scene_aligner")
    lst = []
    for k, f in enumerate(S.stream_s_double_mm()):
        p = tmp_path / f"d{k}.pgm"
        write_pgm16(str(p), f)
        lst.append(f"{k * 0.033:.3f} {p}")
    (tmp_path / "conf.txt").write_text(CONF)
    (tmp_path / "list.txt").write_text("\n".join(lst) + "\n")
    subprocess.check_call([exe, str(tmp_path / "conf.txt"), str(tmp_path / "list.txt"), str(tmp_path / "composed")], timeout=120)
    subprocess.check_call([exe, str(tmp_path / "conf.txt"), str(tmp_path / "list.txt"), str(tmp_path / "one"), "--one-call"], timeout=120)
    a, b = (tmp_path / "composed_trajectory.txt").read_bytes(), (tmp_path / "one_trajectory.txt").read_bytes()
    assert len(a.splitlines()) == S.N_FRAMES and a == b
