"""The merged closure on the GPU: pwn_hip_merge_depth_images against the numpy model of Merger2::mergeDepthImage, bit for bit;
pwn_hip_project_merge_batch against the oracle's projections and the model; PwnCloserWithMerger.processPartition against the same steps
composed by hand from the public calls that existed before it; refusals; the C++ mirror's check tool."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merged_partition as M      # noqa: E402
from conftest import case_params      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPES = [(1, 1), (1, 65), (7, 63), (9, 65), (17, 129), (60, 80), (120, 160)]
COUNTS = [1, 2, 7, 8, 9, 17]


@pytest.fixture(scope="module")
def ctx():
    from g2o_frontend_amd import api
    c = api.Context(device=0, max_rows=120, max_cols=160, max_batch=17, omega_storage="exact9")
    yield c
    c.close()


class Shifted:
    """a device pointer `floats` elements into a DeviceBuffer"""

    def __init__(self, buf, floats, shape):
        self.buf, self._off, self.shape = buf, 4 * floats, shape

    def data_ptr(self): return self.buf.data_ptr() + self._off
    def is_contiguous(self): return True


def ptr(x):
    from g2o_frontend_amd import api
    return api._ptr(x)


def gpu_merge(ctx, images, out, weights, points=0, want_overlap=True):
    """pwn_hip_merge_depth_images -> (status, overlap, points); out / weights are written in place"""
    n = len(images)
    rows, cols = out.shape
    ptrs = (C.c_void_p * max(1, n))(*[ptr(d) for d in images])
    overlap = (C.c_int * max(1, n))(*([-7] * max(1, n)))
    pts = C.c_int(points)
    rc = ctx._L.pwn_hip_merge_depth_images(ctx.h, n, ptrs, rows, cols, ptr(out), ptr(weights), overlap if want_overlap else None, C.byref(pts))
    return rc, np.array(list(overlap)[:n], np.int32), pts.value


def assert_same(got_out, got_w, overlap, points, want, what):
    assert np.array_equal(M.bits(got_out), M.bits(want[0])), what
    assert np.array_equal(M.bits(got_w), M.bits(want[1])), what
    assert np.array_equal(overlap, want[2]), what
    assert points == want[3], what


def natural_planes(rows, cols, n):
    c = M.natural_case() if (rows, cols) == (60, 80) else M.natural_case(rows, cols, case_params("small")[2])
    return [c["planes"][i % len(c["planes"])] for i in range(n)]


# --------------------------------------------------------------------------------------------- pwn_hip_merge_depth_images
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_merge_depth_images_injected_planes_bit_exact(ctx, rows, cols):
    """every shape x every n, host pointers and device pointers, pre-filled merged / weights (the injected case fills them)"""
    for n in COUNTS:
        c = M.injected_case(rows, cols, n)
        want = M.merge_images(c["out"], c["weights"], c["planes"])
        out, w = c["out"].copy(), c["weights"].copy()                          # pageable host memory
        rc, overlap, points = gpu_merge(ctx, c["planes"], out, w)
        assert rc == 0
        assert_same(out, w, overlap, points, want, ("host", rows, cols, n))
        dout, dw = ctx.upload(c["out"]), ctx.upload(c["weights"])              # device memory, images mixed device / host
        dimgs = [ctx.upload(p) if i % 3 != 2 else p for i, p in enumerate(c["planes"])]
        rc, overlap, points = gpu_merge(ctx, dimgs, dout, dw, points=5)
        assert rc == 0
        assert_same(dout.numpy(), dw.numpy(), overlap, points - 5, want, ("device", rows, cols, n))     # points accumulates


@pytest.mark.parametrize("rows,cols", [(60, 80), (120, 160)])
def test_merge_depth_images_natural_planes_bit_exact(ctx, oracle, rows, cols):
    z = np.zeros((rows, cols), F)
    for n in COUNTS:
        planes = natural_planes(rows, cols, n)
        want = M.merge_images(z, z, planes)
        out, w = z.copy(), z.copy()
        rc, overlap, points = gpu_merge(ctx, planes, out, w)
        assert rc == 0
        assert_same(out, w, overlap, points, want, (rows, cols, n))


def test_merge_depth_images_device_pointers_off_a_16_byte_boundary(ctx, oracle):
    rows, cols = 60, 80
    N = rows * cols
    planes = natural_planes(rows, cols, 8)
    inj = M.injected_case(rows, cols, 2)
    z = np.zeros((rows, cols), F)
    for imgs, o0, w0 in ((planes, z, z), (inj["planes"], inj["out"], inj["weights"])):
        want = M.merge_images(o0, w0, imgs)
        pad = lambda a: np.concatenate([np.zeros(1, F), np.asarray(a, F).reshape(-1), np.zeros(3, F)])      # noqa: E731
        bout, bw = ctx.upload(pad(o0)), ctx.upload(pad(w0))
        bimgs = [ctx.upload(pad(p)) for p in imgs]
        assert bout.data_ptr() % 16 == 0
        sh = lambda b: Shifted(b, 1, (rows, cols))      # noqa: E731
        rc, overlap, points = gpu_merge(ctx, [sh(b) for b in bimgs], sh(bout), sh(bw))
        assert rc == 0
        got_o, got_w = bout.numpy(), bw.numpy()
        assert_same(got_o[1:1 + N].reshape(rows, cols), got_w[1:1 + N].reshape(rows, cols), overlap, points, want, "shifted")
        assert not got_o[0] and not got_o[1 + N:].any() and not got_w[0] and not got_w[1 + N:].any()      # nothing written around the images


def test_merge_depth_images_split_call_equals_one_call(ctx, oracle):
    rows, cols = 60, 80
    planes = natural_planes(rows, cols, 8)
    z = np.zeros((rows, cols), F)
    one_o, one_w = ctx.upload(z), ctx.upload(z)
    rc, ov8, p8 = gpu_merge(ctx, planes, one_o, one_w)
    assert rc == 0
    two_o, two_w = ctx.upload(z), ctx.upload(z)
    rc, ov3, p3 = gpu_merge(ctx, planes[:3], two_o, two_w)
    assert rc == 0
    rc, ov5, p35 = gpu_merge(ctx, planes[3:], two_o, two_w, points=p3)
    assert rc == 0
    assert np.array_equal(M.bits(one_o.numpy()), M.bits(two_o.numpy())) and np.array_equal(M.bits(one_w.numpy()), M.bits(two_w.numpy()))
    assert ov8.tolist() == ov3.tolist() + ov5.tolist() and p8 == p35
    assert_same(one_o.numpy(), one_w.numpy(), ov8, p8, M.merge_images(z, z, planes), "8 in one call")
    # counters are optional
    o, w = z.copy(), z.copy()
    n = len(planes)
    ptrs = (C.c_void_p * n)(*[ptr(d) for d in planes])
    assert ctx._L.pwn_hip_merge_depth_images(ctx.h, n, ptrs, rows, cols, ptr(o), ptr(w), None, None) == 0
    assert np.array_equal(M.bits(o), M.bits(one_o.numpy()))


def test_merge_depth_images_in_chunks_of_three_planes(oracle):
    """a context whose scratch holds 3 planes takes 8 images -- host ones staged through plane i % 3 of their chunk, device ones read in
    place -- with the bits of the model"""
    from g2o_frontend_amd import api
    rows, cols = 60, 80
    small = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=3)
    try:
        planes = natural_planes(rows, cols, 8)
        inj = M.injected_case(rows, cols, 8)
        z = np.zeros((rows, cols), F)
        for imgs, o0, w0 in ((planes, z, z), (inj["planes"], inj["out"], inj["weights"])):
            want = M.merge_images(o0, w0, imgs)
            for device in ((), (1, 3, 4), range(8)):                        # all host, mixed, all device
                mixed = [small.upload(p) if i in device else p for i, p in enumerate(imgs)]
                out, w = o0.copy(), w0.copy()
                rc, overlap, points = gpu_merge(small, mixed, out, w)
                assert rc == 0
                assert_same(out, w, overlap, points, want, ("chunks", tuple(device)))
                del mixed
    finally:
        small.close()


def test_device_memset_clears_a_device_image(ctx):
    buf = ctx.upload(np.arange(1, 1001, dtype=F))
    buf.zero()
    assert not buf.numpy().any()
    assert ctx._L.pwn_hip_device_memset(None, None, 0, 4) == 1 and ctx._L.pwn_hip_device_memset(ctx.h, ptr(np.zeros(4, F)), 0, 16) == 1


# -------------------------------------------------------------------------------------------- pwn_hip_project_merge_batch
def upload_cloud(ctx, ocloud):
    from g2o_frontend_amd import api
    a = ocloud.arrays()
    c = api.Cloud(ctx, max(1, len(ocloud)))
    c.upload(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])
    return c


def project_merge(ctx, K, clouds, transforms, rows, cols, out, weights, want_planes=True, points=0):
    n = len(clouds)
    Kc = np.array([K[0], 0, 0, 0, K[1], 0, K[2], K[3], 1], F)
    handles = (C.c_void_p * max(1, n))(*[c.h for c in clouds])
    tr = np.ascontiguousarray(np.stack([np.asarray(T, F).T.reshape(-1) for T in transforms]), F)
    overlap = (C.c_int * max(1, n))(); pts = C.c_int(points)
    planes = np.full((n, rows, cols), -1, F) if want_planes else None
    rc = ctx._L.pwn_hip_project_merge_batch(ctx.h, ptr(Kc), n, handles, ptr(tr), M.MIN_DISTANCE, M.MAX_DISTANCE, rows, cols, ptr(out), ptr(weights), overlap,
                                            C.byref(pts), ptr(planes))
    return rc, planes, np.array(list(overlap)[:n], np.int32), pts.value


def batch_of_eight(ctx, oracle, case):
    """eight clouds: natural ones, an empty one, one wholly behind the camera, two identical -> (gpu clouds, transforms, the oracle's planes)"""
    from g2o_frontend_amd import api
    rows, cols, K = case["rows"], case["cols"], case["K"]
    oc, tr = case["clouds"], case["transforms"]
    behind = tr[3] @ np.diag([-1, 1, -1, 1]).astype(F)                      # the projector turned by 180 degrees about y
    order = [(0, tr[0]), (1, tr[1]), (None, tr[2]), (2, tr[2]), (2, tr[2]), (3, behind), (4, tr[4]), (5, tr[5])]
    up = {k: upload_cloud(ctx, oc[k]) for k in range(6)}
    empty = api.Cloud(ctx, 64)
    clouds = [empty if k is None else up[k] for k, _ in order]
    planes = [np.full((rows, cols), M.FLT_MAX, F) if k is None else oracle.project(K, T, M.MIN_DISTANCE, M.MAX_DISTANCE, rows, cols, case["points"][k])[1]
              for k, T in order]
    assert (planes[5] == M.FLT_MAX).all() and (planes[3] < M.FLT_MAX).any()
    return clouds, [T for _, T in order], planes


@pytest.mark.parametrize("rows,cols", [(60, 80), (120, 160)])
def test_project_merge_batch_against_the_oracle_and_the_model(ctx, oracle, rows, cols):
    from g2o_frontend_amd import api
    case = M.natural_case() if rows == 60 else M.natural_case(rows, cols, case_params("small")[2])
    K = case["K"]
    clouds, transforms, oplanes = batch_of_eight(ctx, oracle, case)
    z = np.zeros((rows, cols), F)
    want = M.merge_images(z, z, oplanes)
    out, w = ctx.upload(z), ctx.upload(z)
    rc, planes, overlap, points = project_merge(ctx, K, clouds, transforms, rows, cols, out, w)
    assert rc == 0
    for k in range(8):
        assert np.array_equal(M.bits(planes[k]), M.bits(oplanes[k])), k
    assert_same(out.numpy(), w.numpy(), overlap, points, want, "batch")
    # a context whose scratch holds 3 planes: the same bits in chunks (its clouds are its own)
    small = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=3, omega_storage="exact9")
    try:
        sclouds, _, _ = batch_of_eight(small, oracle, case)
        o3, w3 = z.copy(), z.copy()
        rc, planes3, overlap3, points3 = project_merge(small, K, sclouds, transforms, rows, cols, o3, w3)
        assert rc == 0
        assert np.array_equal(M.bits(planes3), M.bits(planes))
        assert_same(o3, w3, overlap3, points3, want, "chunks of 3")
        del sclouds
    finally:
        small.close()
    # n pwn_hip_project calls followed by pwn_hip_merge_depth_images
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]); proj.setMinDistance(M.MIN_DISTANCE); proj.setMaxDistance(M.MAX_DISTANCE)
    proj.setImageSize(rows, cols)
    singles = []
    for c, T in zip(clouds, transforms):
        proj.setTransform(T)
        singles.append(proj.project(c)[1])
        assert np.array_equal(M.bits(singles[-1]), M.bits(planes[len(singles) - 1]))
    o1, w1 = z.copy(), z.copy()
    rc, ov1, p1 = gpu_merge(ctx, singles, o1, w1)
    assert rc == 0
    assert_same(o1, w1, ov1, p1, want, "project + merge")
    # without the planes, host outputs, pre-filled images
    inj = M.injected_case(rows, cols, 1)
    o2, w2 = inj["out"].copy(), inj["weights"].copy()
    rc, none, ov2, p2 = project_merge(ctx, K, clouds, transforms, rows, cols, o2, w2, want_planes=False, points=11)
    assert rc == 0 and none is None
    assert_same(o2, w2, ov2, p2 - 11, M.merge_images(inj["out"], inj["weights"], oplanes), "pre-filled")


def test_project_merge_batch_vga_once(oracle):
    from g2o_frontend_amd import api, synth
    rows, cols, K = 480, 640, synth.K_VGA
    case = M.natural_case(rows, cols, K)
    vga = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=8, omega_storage="exact9")
    try:
        clouds = [upload_cloud(vga, c) for c in case["clouds"]]
        z = np.zeros((rows, cols), F)
        out, w = vga.upload(z), vga.upload(z)
        rc, planes, overlap, points = project_merge(vga, K, clouds, case["transforms"], rows, cols, out, w)
        assert rc == 0
        for k in range(8):
            assert np.array_equal(M.bits(planes[k]), M.bits(case["planes"][k])), k
        assert_same(out.numpy(), w.numpy(), overlap, points, M.merge_images(z, z, case["planes"]), "vga")
        del clouds, out, w
    finally:
        vga.close()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(ctx, oracle):
    from g2o_frontend_amd import api
    rows, cols = 60, 80
    case = M.natural_case()
    K = np.array([case["K"][0], 0, 0, 0, case["K"][1], 0, case["K"][2], case["K"][3], 1], F)
    cloud = upload_cloud(ctx, case["clouds"][0])
    other_ctx = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=1)
    foreign = api.Cloud(other_ctx, 16)
    inj = M.injected_case(rows, cols, 1)
    out, w = inj["out"].copy(), inj["weights"].copy()
    dout, dw = ctx.upload(out), ctx.upload(w)
    overlap = (C.c_int * 2)(-3, -3); pts = C.c_int(17)
    img = case["planes"][0]
    imgs = (C.c_void_p * 2)(ptr(img), ptr(img)); holes = (C.c_void_p * 2)(ptr(img), None)
    big, big2 = np.zeros((200, 200), F), np.zeros((200, 200), F)
    tr = np.ascontiguousarray(np.stack([np.eye(4, dtype=F).reshape(-1)] * 2))
    h_ok = (C.c_void_p * 2)(cloud.h, cloud.h); h_null = (C.c_void_p * 2)(cloud.h, None); h_foreign = (C.c_void_p * 2)(cloud.h, foreign.h)
    L = ctx._L
    INVALID, CAPACITY = 1, 6
    for o, wt in ((out, w), (dout, dw)):
        merges = [
            (INVALID, (ctx.h, 2, None, rows, cols, ptr(o), ptr(wt), overlap, C.byref(pts))),
            (INVALID, (ctx.h, 2, holes, rows, cols, ptr(o), ptr(wt), overlap, C.byref(pts))),
            (INVALID, (ctx.h, 2, imgs, rows, cols, None, ptr(wt), overlap, C.byref(pts))),
            (INVALID, (ctx.h, 2, imgs, rows, cols, ptr(o), None, overlap, C.byref(pts))),
            (INVALID, (ctx.h, -1, imgs, rows, cols, ptr(o), ptr(wt), overlap, C.byref(pts))),
            (INVALID, (ctx.h, 2, imgs, rows, cols, ptr(o), ptr(o), overlap, C.byref(pts))),      # merged == weights
            (INVALID, (None, 2, imgs, rows, cols, ptr(o), ptr(wt), overlap, C.byref(pts))),
            (CAPACITY, (ctx.h, 2, imgs, 200, 200, ptr(big), ptr(big2), overlap, C.byref(pts))),
            (CAPACITY, (ctx.h, 2, imgs, 1, 19200, ptr(o), ptr(wt), overlap, C.byref(pts))),
            (INVALID, (ctx.h, 2, imgs, 0, cols, ptr(o), ptr(wt), overlap, C.byref(pts))),
        ]
        for want, args in merges:
            assert L.pwn_hip_merge_depth_images(*args) == want, args
        tail = lambda: (ptr(o), ptr(wt), overlap, C.byref(pts), None)      # noqa: E731
        batches = [
            (INVALID, (ctx.h, None, 2, h_ok, ptr(tr), 0.01, 6.0, rows, cols) + tail()),
            (INVALID, (ctx.h, ptr(K), 2, None, ptr(tr), 0.01, 6.0, rows, cols) + tail()),
            (INVALID, (ctx.h, ptr(K), 2, h_ok, None, 0.01, 6.0, rows, cols) + tail()),
            (INVALID, (ctx.h, ptr(K), 2, h_null, ptr(tr), 0.01, 6.0, rows, cols) + tail()),
            (INVALID, (ctx.h, ptr(K), 2, h_foreign, ptr(tr), 0.01, 6.0, rows, cols) + tail()),
            (INVALID, (ctx.h, ptr(K), -2, h_ok, ptr(tr), 0.01, 6.0, rows, cols) + tail()),
            (INVALID, (ctx.h, ptr(K), 2, h_ok, ptr(tr), -0.01, 6.0, rows, cols) + tail()),
            (CAPACITY, (ctx.h, ptr(K), 2, h_ok, ptr(tr), 0.01, 6.0, 121, 161) + tail()),
            (INVALID, (ctx.h, ptr(K), 2, h_ok, ptr(tr), 0.01, 6.0, rows, cols, None, ptr(wt), overlap, C.byref(pts), None)),
        ]
        for want, args in batches:
            assert L.pwn_hip_project_merge_batch(*args) == want, args
        assert ctx._L.pwn_hip_last_error_string(ctx.h)
        # n == 0: success, nothing written
        assert L.pwn_hip_merge_depth_images(ctx.h, 0, None, rows, cols, ptr(o), ptr(wt), overlap, C.byref(pts)) == 0
        assert L.pwn_hip_project_merge_batch(ctx.h, ptr(K), 0, None, None, 0.01, 6.0, rows, cols, ptr(o), ptr(wt), overlap, C.byref(pts), None) == 0
    assert list(overlap) == [-3, -3] and pts.value == 17
    assert np.array_equal(M.bits(out), M.bits(inj["out"])) and np.array_equal(M.bits(w), M.bits(inj["weights"]))
    assert np.array_equal(M.bits(dout.numpy()), M.bits(inj["out"])) and np.array_equal(M.bits(dw.numpy()), M.bits(inj["weights"]))
    assert not big.any() and not big2.any()
    del foreign
    other_ctx.close()


# ------------------------------------------------------------------------------------------------------- the closure end to end
E2E_SEED, E2E_YAW = 3, 35.0
E2E_MIN_NON_ZERO = 20000          # half of it, 10 000 pixels, is a little over half of the 120 x 160 image: the aligned view passes, the turned one does not


def closure_objects(ctx):
    """the object graph of the closer at 120 x 160: projector range (0.01, 6), matcher at scale 1"""
    from g2o_frontend_amd import api
    from test_gpu_parity import gpu_objects
    proj, converter, aligner = gpu_objects(ctx, "small")
    proj.setMinDistance(M.MIN_DISTANCE); proj.setMaxDistance(M.MAX_DISTANCE)
    matcher = api.PwnMatcherBase(aligner, converter)
    matcher.setScale(1)
    return proj, converter, aligner, matcher


def turned(pose, yaw_deg):
    a = np.deg2rad(yaw_deg)
    R = np.eye(4); R[0, 0] = np.cos(a); R[0, 2] = np.sin(a); R[2, 0] = -np.sin(a); R[2, 2] = np.cos(a)
    return pose @ R


def closure_input(yaw_deg):
    """nine keyframes of the seeded room: frame 0 (turned by yaw_deg about its y axis) is `current`, frames 1-8 the other partition"""
    from g2o_frontend_amd import synth
    from oracle import oracle as O
    rows, cols, K, _, _ = case_params("small")
    frames, poses = M.room_frames(E2E_SEED, 9, rows, cols, K)
    poses = [p.copy() for p in poses]; frames = list(frames)
    if yaw_deg:
        poses[0] = turned(poses[0], yaw_deg)
        frames[0] = O.convert_16u_to_32f(synth.render_depth_mm(E2E_SEED, poses[0], rows, cols, K, hole_stream=0))
    return rows, cols, K, frames, poses


@pytest.mark.parametrize("yaw,accepted", [(0.0, True), (E2E_YAW, False)])
def test_process_partition_equals_the_steps_composed_by_hand(ctx, oracle, yaw, accepted):
    from g2o_frontend_amd import api
    rows, cols, K, frames, poses = closure_input(yaw)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], F)
    offset = np.eye(4)
    proj, converter, aligner, matcher = closure_objects(ctx)
    cache = api.CloudCache(matcher, capacity=16)
    nodes = [api.MapNode(k, poses[k], offset) for k in range(9)]
    for k in range(9):
        cache.addFrame(k, frames[k], Km, offset.astype(F))
    merger = api.Merger2(ctx, converter, matcher)
    closer = api.PwnCloserWithMerger(merger, cache, frameMinNonZeroThreshold=E2E_MIN_NON_ZERO)
    current, others = nodes[0], nodes[1:]
    relations = closer.processPartition(others, current)
    result = dict(merger._result)
    fused_gpu = closer._otherPartitionImage.numpy(); current_gpu = closer._currentPartitionImage.numpy()
    fused_cloud = merger._bigCloud.arrays()
    counts = (merger._image_points_count, merger._image_overlapping_points_count, list(merger.overlaps))
    assert closer.accepted is accepted
    assert closer.processPartition(nodes, current) == [] and closer.accepted is None      # `current` inside the other partition (:113-114)

    # the same steps from the calls that existed before: per-cloud projection, the numpy model, compute, matchClouds
    proj2, converter2, aligner2, matcher2 = closure_objects(ctx)
    z = np.zeros((rows, cols), F)
    proj2.setImageSize(rows, cols)

    def plane(node, T):
        proj2.setCameraMatrix(Km); proj2.setTransform(np.asarray(T, np.float64).astype(F))
        return proj2.project(cache.get(node.key))[1]
    current_img = M.merge_images(z, z, [plane(current, offset)])[0]
    # the mirror composes the projector transforms with loops in a fixed order, the model with numpy's products: equal once cast to float32
    for o in others:
        assert np.array_equal(M.bits(closer.projectorTransform(o, current, o.sensorOffset)), M.bits(M.projector_transform(o.transform(), current.transform(), offset)))
    planes = [plane(o, M.projector_transform(o.transform(), current.transform(), offset)) for o in others]
    fused, _, overlap, points, _ = M.merge_images(z, z, planes)
    assert np.array_equal(M.bits(current_gpu), M.bits(current_img)) and np.array_equal(M.bits(fused_gpu), M.bits(fused))
    assert counts == (points, int(overlap[-1]), overlap.tolist())
    node_list = [o for o, c in zip(others, overlap) if c > 4000]
    assert node_list and [o.key for o in closer._nodeList] == [o.key for o in node_list]
    big, cur_big = api.Cloud(ctx, rows * cols), api.Cloud(ctx, rows * cols)
    converter2.compute(big, fused, offset.astype(F)); converter2.compute(cur_big, current_img, offset.astype(F))
    aligner2.clearPriors()
    want = matcher2.matchClouds(cur_big, big, offset.astype(F), offset.astype(F), Km, rows, cols, np.eye(4))
    for key in ("image_nonZeros", "image_outliers", "image_inliers", "cloud_inliers"):
        assert result[key] == want[key], key
    assert F(result["image_reprojectionDistance"]).view(np.uint32) == F(want["image_reprojectionDistance"]).view(np.uint32)
    assert np.array_equal(result["transform"], want["transform"])
    assert np.array_equal(M.bits(result["align"]["chi2"]), M.bits(want["align"]["chi2"])) and result["align"]["inliers"] == want["align"]["inliers"]
    assert M.rejected(want["image_nonZeros"], want["image_outliers"], want["image_inliers"], minNonZero=E2E_MIN_NON_ZERO) is (not accepted)
    # the fused cloud is the oracle's conversion of the model's fused image (the context stores exact9)
    from test_gpu_parity import oracle_params
    cp, _ = oracle_params(oracle, "small")
    cp.min_distance, cp.max_distance = M.MIN_DISTANCE, M.MAX_DISTANCE
    oc = oracle.convert(cp, fused)[0].arrays()
    for key in ("points", "normals", "curvature", "omega_p", "omega_n"):
        assert np.array_equal(M.bits(fused_cloud[key]), M.bits(oc[key])), key
    # the relations
    if accepted:
        assert len(relations) == len(node_list)
        for r, nodo in zip(relations, node_list):
            assert r["nodes"][0] is current and r["nodes"][1] is nodo
            T = M.relation_transform(current.transform(), current.transform(), want["transform"], nodo.transform())
            assert np.allclose(r["transform"], T, rtol=0, atol=1e-12)
            assert np.array_equal(r["informationMatrix"], M.INFORMATION)
            assert r["image_inliers"] == want["image_inliers"]
            # the relation puts nodo where the trajectory has it, to the accuracy of the alignment
            assert np.abs(r["transform"] - np.linalg.inv(current.transform()) @ nodo.transform()).max() < 2e-2
    else:
        assert relations == []


# -------------------------------------------------------------------------------------------------------- the C++ check tool
def write_closure_file(path, rows, cols, K, frames, poses, min_non_zero, accepted, relations):
    """the input of tools/pwn_hip_merged_closure_check: sizes, camera, thresholds, the frames and poses, then what the Python mirror returned"""
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", rows, cols, len(frames), int(min_non_zero)))
        f.write(np.asarray(K, np.float64).tobytes())
        for fr, p in zip(frames, poses):
            f.write(np.asarray(p, np.float64).tobytes())                    # row-major 4 x 4
            f.write(np.ascontiguousarray(fr, F).tobytes())
        f.write(struct.pack("<2i", -1 if accepted is None else int(accepted), len(relations)))
        for r in relations:
            f.write(struct.pack("<2i", r["nodes"][0].key, r["nodes"][1].key))
            f.write(np.asarray(r["transform"], np.float64).tobytes())
            f.write(struct.pack("<3i", r["image_nonZeros"], r["image_outliers"], r["image_inliers"]))


@pytest.mark.parametrize("yaw,accepted", [(0.0, True), (E2E_YAW, False)])
def test_cpp_mirror_gives_the_python_mirrors_relations(ctx, oracle, tmp_path, yaw, accepted):
    from g2o_frontend_amd import api, build
    build.build_tools()
    rows, cols, K, frames, poses = closure_input(yaw)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], F)
    proj, converter, aligner, matcher = closure_objects(ctx)
    cache = api.CloudCache(matcher, capacity=16)
    nodes = [api.MapNode(k, poses[k]) for k in range(9)]
    for k in range(9):
        cache.addFrame(k, frames[k], Km, np.eye(4, dtype=F))
    closer = api.PwnCloserWithMerger(api.Merger2(ctx, converter, matcher), cache, frameMinNonZeroThreshold=E2E_MIN_NON_ZERO)
    relations = closer.processPartition(nodes[1:], nodes[0])
    assert closer.accepted is accepted
    path = str(tmp_path / "closure.bin")
    write_closure_file(path, rows, cols, K, frames, poses, E2E_MIN_NON_ZERO, closer.accepted, relations)
    r = subprocess.run([os.path.join(ROOT, "tools", "pwn_hip_merged_closure_check"), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 differences" in r.stdout
