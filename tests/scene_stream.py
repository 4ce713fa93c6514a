"""The inputs of the mapping-step tests (pwn_hip_scene_step), at 120x160 (case_params("small")), and the oracle's run of the loop of
pwn_aligner.cpp:166-209 over them.  test_scene_stream_cpu.py holds the generator to what the GPU tests rely on.

Stream S: synth.trajectory(3, 5) rendered with render_depth_mm(3, pose, ..., hole_stream=k); frame 3 replaced by an all-zero frame.
  The blank frame converts to m = 0 points, so the scene's size n and the step's upper bound n + rows * cols fall into different 1024-blocks
  of the scan; it follows a larger step, so stale scratch lies beyond n; frame 4 is natural again.
Stream W: frames 0, 2, 4 of the unmodified stream (stream_wide).
Case H: frame 0 with columns >= 80 zeroed makes the scene, frame 1 with columns < 88 zeroed is the step: the rendering of the scene and the
  frame share no pixel, the aligner returns the identity with 0 inliers, and Cloud::add's identity branch runs on a pose the device computed.
"""
import numpy as np

from conftest import case_params

NAME = "small"
SEED = 3
N_FRAMES = 5
BLANK = 3


def stream_mm(rows, cols, K, blank=True):
    """the five uint16 millimetre frames of stream S at the given size and camera"""
    from g2o_frontend_amd import synth
    poses = synth.trajectory(SEED, N_FRAMES)
    frames = [synth.render_depth_mm(SEED, poses[k], rows, cols, K, hole_stream=k) for k in range(N_FRAMES)]
    if blank:
        frames[BLANK] = np.zeros_like(frames[BLANK])
    return frames


def stream_s(oracle, blank=True):
    """stream S as float32 metres at 120x160"""
    rows, cols, K, _, _ = case_params(NAME)
    return [oracle.convert_16u_to_32f(f) for f in stream_mm(rows, cols, K, blank)]


def stream_wide(oracle):
    """frames 0, 2 and 4 of the unmodified stream: twice the motion per step.  On stream S the aligner's reference projections put two points
    into one pixel in frame 4 only (the step behind the blank frame, which sees that motion); here they do in every step."""
    return stream_s(oracle, blank=False)[::2]


def stream_s_double_mm():
    """stream S rendered at 240x320 (uint16 millimetres): DepthImage_scale with step 2 brings it to the case's size and camera"""
    from g2o_frontend_amd import synth
    rows, cols, _, _, _ = case_params(NAME)
    return stream_mm(2 * rows, 2 * cols, synth.scaled_K(synth.K_VGA, 2), True)


def case_h(oracle):
    """(the frame that makes the scene, the frame of the step)"""
    a, b = stream_s(oracle, blank=False)[:2]
    a, b = a.copy(), b.copy()
    a[:, 80:] = 0
    b[:, :88] = 0
    return a, b


def oracle_loop(oracle, depths, sensor_offset=None):
    """The mapping loop on the oracle, free-running (accumulate_fp64 = 1): per frame a dict with the clouds' sizes, the aligner's result, the
    scene pose, the scene's size after the add and after the merge, and _collapsedIndices."""
    from test_gpu_parity import oracle_params
    rows, cols, K, conv, _ = case_params(NAME)
    cp, ap = oracle_params(oracle, NAME, sensor_offset=sensor_offset, accumulate_fp64=1)
    so = np.eye(4, dtype=np.float32) if sensor_offset is None else np.asarray(sensor_offset, np.float32)
    scene = oracle.Cloud()
    sceneT = np.eye(4, dtype=np.float32)
    out = []
    oracle.set_gaussians(True)
    try:
        for d in depths:
            cloud, _, _ = oracle.convert(cp, d)
            view = oracle.iso_mul(sceneT, so)
            _, dep = oracle.project(K, view, conv["min_distance"], conv["max_distance"], rows, cols, scene.arrays()["points"])
            sub, _, _ = oracle.convert(cp, dep)
            res = oracle.align(ap, sub, cloud)
            sceneT = oracle.iso_mul(sceneT, res["T"])
            sceneT[3] = (0, 0, 0, 1)
            scene.add(cloud, sceneT)
            n_add = len(scene)
            k, col = oracle.merge(scene, K, oracle.iso_mul(sceneT, so), conv["min_distance"], conv["max_distance"], rows, cols)
            out.append(dict(n_cloud=len(cloud), n_subscene=len(sub), align=res, sceneT=sceneT.copy(), size_add=n_add, size_merge=k, collapsed=col))
    finally:
        oracle.set_gaussians(False)
    return out
