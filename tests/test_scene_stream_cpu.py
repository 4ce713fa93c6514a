"""No GPU: the oracle alone proves what tests/scene_stream.py claims about its inputs, and the library built here exports the mapping step
with the structs the header declares (test_gpu_scene_step.py runs it)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import scene_stream as S
from conftest import case_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def natural_loop(oracle):
    return S.oracle_loop(oracle, S.stream_s(oracle, blank=False))


def test_every_natural_frame_fuses_and_leaves_points_outside_the_view(natural_loop):
    """Measured on the CPU, free-running with accumulate_fp64 = 1: at least 17 093 fused points and 1 005 points with collapsed == -1 per frame."""
    assert len(natural_loop) == S.N_FRAMES
    for k, f in enumerate(natural_loop[1:], 1):
        col = f["collapsed"]
        fused = int(((col >= 0) & (col != np.arange(len(col)))).sum())
        outside = int((col == -1).sum())
        print(k, "fused", fused, "collapsed == -1", outside, "sizes", f["n_cloud"], f["n_subscene"], f["size_add"], f["size_merge"])
        assert fused >= 10000, (k, fused)
        assert outside >= 500, (k, outside)
        assert f["size_add"] - f["size_merge"] == fused


def test_the_blank_frame_converts_to_no_points(oracle):
    from test_gpu_parity import oracle_params
    frames = S.stream_s(oracle)
    assert not frames[S.BLANK].any() and all(f.any() for k, f in enumerate(frames) if k != S.BLANK)
    cp, _ = oracle_params(oracle, S.NAME)
    cloud, idx, _ = oracle.convert(cp, frames[S.BLANK])
    assert len(cloud) == 0 and np.all(idx == -1)


def test_the_blank_frame_puts_size_and_bound_into_different_scan_blocks(oracle):
    """the scan of the keep flags runs over size + rows * cols entries in blocks of 1024"""
    rows, cols, _, _, _ = case_params(S.NAME)
    f = S.oracle_loop(oracle, S.stream_s(oracle))[S.BLANK]
    assert f["n_cloud"] == 0 and f["size_add"] // 1024 != (f["size_add"] + rows * cols - 1) // 1024


def test_case_h_aligns_to_the_identity_with_points(oracle):
    """Measured: 8 399 points in the cloud, 9 314 in the sub-scene."""
    a, b = S.case_h(oracle)
    scene_frame, step = S.oracle_loop(oracle, [a, b])
    res = step["align"]
    print("cloud", step["n_cloud"], "sub-scene", step["n_subscene"])
    assert np.array_equal(res["T"], np.eye(4, dtype=np.float32)) and res["inliers"] == 0
    assert all(it["inliers"] == 0 for it in res["iterations"])
    assert step["n_cloud"] > 5000 and step["n_subscene"] > 0
    assert np.array_equal(step["sceneT"], np.eye(4, dtype=np.float32))      # the identity branch of Cloud::add


def test_the_library_exports_the_mapping_step():
    from g2o_frontend_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "pwn_hip_scene_step") and hasattr(L, "pwn_hip_default_scene_step_params")
    assert "pwn_hip_scene_step" in _lib.PROTOTYPES


def test_the_step_structs_have_the_headers_sizes():
    from g2o_frontend_amd import _lib
    prog = r'''
#include <stdio.h>
#include "pwn_hip.h"
int main(void) { printf("%zu %zu\n", sizeof(pwn_hip_scene_step_params), sizeof(pwn_hip_scene_step_result)); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    assert [int(x) for x in out] == [C.sizeof(_lib.SceneStepParams), C.sizeof(_lib.SceneStepResult)]
    p = _lib.SceneStepParams()
    _lib.lib().pwn_hip_default_scene_step_params(C.byref(p))
    assert (round(p.distance_threshold, 6), round(p.max_point_depth, 6), round(p.baseline, 6), round(p.alpha, 6), p.step) == (0.1, 10.0, 0.075, 0.1, 0)
    assert abs(p.normal_threshold - np.cos(np.deg2rad(10))) < 1e-6
