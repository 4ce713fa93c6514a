"""pwn_hip_scene_step (one frame of the mapping loop of pwn_aligner.cpp:166-209 in one submission) against the composed route on a second set
of clouds in the same context: pwn_hip_convert_batch_ex, pwn_hip_project into a device image, pwn_hip_convert_batch of that image, pwn_hip_align,
pwn_hip_iso_mul with the last row forced, pwn_hip_cloud_add, pwn_hip_merge.  After every frame the same bytes are required in every downloaded
array of the three clouds (Stats, Gaussians with flags and the Gaussian tail included), in the align result (its time apart), in the scene pose,
all counts and _collapsedIndices.  The composed route is held to the oracle frame by frame by test_scene.py::test_incremental_scene_harness;
tests/scene_stream.py has the inputs, test_scene_stream_cpu.py what they are chosen for."""
import ctypes as C

import numpy as np
import pytest

import scene_stream as S
from conftest import case_params
from test_scene import OFFSET

pytestmark = pytest.mark.gpu

AWAY = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, -10], [0, 0, 0, 1]], np.float32)      # the `away` view of test_scene.py
ALIGN_FIELDS = ("T", "error", "inliers", "iterations", "chi2", "iter_inliers", "iter_correspondences", "iter_candidates", "n_reference", "n_current")      # not the time


@pytest.fixture(scope="module")
def contexts():
    from g2o_frontend_amd import api
    made = {}

    def get(storage):
        if storage not in made:
            made[storage] = api.Context(device=0, max_rows=240, max_cols=320, max_batch=2, omega_storage=storage)
        return made[storage]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def frames(oracle):
    return dict(S=S.stream_s(oracle), W=S.stream_wide(oracle), H=list(S.case_h(oracle)), S2=S.stream_s_double_mm())


class Params:
    """the converter, aligner and step parameters of the "small" case"""

    def __init__(self, ctx, offset=None, step=0):
        from g2o_frontend_amd import api
        from test_gpu_parity import gpu_objects
        self.rows, self.cols, _, _, _ = case_params(S.NAME)
        self.proj, self.converter, self.aligner = gpu_objects(ctx, S.NAME, sensor_offset=offset)
        self.merger = api.Merger(); self.merger.setDepthImageConverter(self.converter); self.merger.setImageSize(self.rows, self.cols)
        self.offset = np.eye(4, dtype=np.float32) if offset is None else np.asarray(offset, np.float32)
        self.cp = self.converter.params(offset)
        self.aligner.setInitialGuess(np.eye(4, dtype=np.float32))
        self.ap = self.aligner.params()
        self.sp = api.SceneStepParams()
        ctx._L.pwn_hip_default_scene_step_params(C.byref(self.sp))
        self.sp.normal_threshold = self.merger.normalThreshold()
        self.sp.step = step


class Clouds:
    """scene, cloud and sub-scene of one route, and its scene pose"""

    def __init__(self, ctx, pixels, capacity=None):
        from g2o_frontend_amd import api
        self.scene = api.Cloud(ctx, capacity if capacity is not None else (S.N_FRAMES + 1) * pixels)
        self.cloud, self.sub = api.Cloud(ctx, pixels), api.Cloud(ctx, pixels)
        self.sceneT = np.eye(4, dtype=np.float32)

    @classmethod
    def of(cls, scene, cloud, sub):
        w = cls.__new__(cls)
        w.scene, w.cloud, w.sub, w.sceneT = scene, cloud, sub, None
        return w

    def snapshot(self):
        out = {}
        for name, c, stats in (("scene", self.scene, True), ("cloud", self.cloud, True), ("subscene", self.sub, False)):
            out[name + ".size"] = c.size()
            if c.size() > 0:
                for k, a in c.arrays(stats=stats).items():
                    out[name + "." + k] = a.tobytes()
            out[name + ".gaussians"] = c.numGaussians()
            if c.numGaussians() > 0:
                for k, a in c.gaussians().items():
                    out[name + ".gauss." + k] = a.tobytes()
        return out


def _mul(L, A, B):
    from g2o_frontend_amd.api import _colmajor, _from_colmajor, _ptr
    out = np.empty(16, np.float32)
    L.pwn_hip_iso_mul(_ptr(_colmajor(A, 4)), _ptr(_colmajor(B, 4)), _ptr(out))
    return _from_colmajor(out, 4)


def _align_bytes(r):
    return {f: bytes(getattr(r, f)) if isinstance(getattr(r, f), C.Array) else getattr(r, f) for f in ALIGN_FIELDS}


def composed(ctx, P, W, frame, raw_scale=None):
    """the seven calls; returns what pwn_hip_scene_step returns"""
    from g2o_frontend_amd import api
    from g2o_frontend_amd.api import _colmajor, _ptr
    L = ctx._L
    rows, cols = frame.shape
    vrows, vcols = P.rows, P.cols
    ex = api.ConvertExtras(1, 1, P.sp.baseline, P.sp.alpha)
    ctx.check(L.pwn_hip_convert_batch_ex(ctx.h, C.byref(P.cp), (C.c_void_p * 1)(_ptr(frame)), 0 if raw_scale is None else 1, raw_scale or 0.0, 1, rows, cols,
                                         P.sp.step, P.sp.max_depth_cov, C.byref(ex), (C.c_void_p * 1)(W.cloud.h)))
    K = _colmajor(P.proj.cameraMatrix(), 3)
    image = api.DeviceBuffer(ctx, np.zeros((vrows, vcols), np.float32))
    ctx.check(L.pwn_hip_project(ctx.h, _ptr(K), _ptr(_colmajor(_mul(L, W.sceneT, P.offset), 4)), P.proj.minDistance(), P.proj.maxDistance(), vrows, vcols,
                                W.scene.h, None, _ptr(image)))
    ctx.check(L.pwn_hip_convert_batch(ctx.h, C.byref(P.cp), (C.c_void_p * 1)(_ptr(image)), 1, vrows, vcols, (C.c_void_p * 1)(W.sub.h)))
    image.free()
    res = api.AlignResult()
    ctx.check(L.pwn_hip_align(ctx.h, C.byref(P.ap), W.sub.h, W.cloud.h, C.byref(res)))
    launches = {s: ctx.stage_ms(s)[1] for s in ("project_ref", "project_cur", "corr_linearize", "solve")}
    T = api._from_colmajor(res.T, 4)
    W.sceneT = _mul(L, W.sceneT, T); W.sceneT[3] = (0, 0, 0, 1)
    ctx.check(L.pwn_hip_cloud_add(ctx.h, W.scene.h, W.cloud.h, _ptr(_colmajor(W.sceneT, 4))))
    n_add = W.scene.size()
    collapsed = np.empty(max(n_add, 1), np.int32)
    k = C.c_int(0)
    ctx.check(L.pwn_hip_merge(ctx.h, W.scene.h, _ptr(K), _ptr(_colmajor(_mul(L, W.sceneT, P.offset), 4)), P.proj.minDistance(), P.proj.maxDistance(), vrows, vcols,
                              P.sp.distance_threshold, P.sp.normal_threshold, P.sp.max_point_depth, C.byref(k), _ptr(collapsed)))
    return dict(align=_align_bytes(res), T=T, sceneT=W.sceneT.copy(), n_cloud=W.cloud.size(), n_subscene=W.sub.size(), size_add=n_add, size_merge=k.value,
                collapsed=collapsed[:n_add].copy(), launches=launches)


def one_call(ctx, P, W, frame, raw_scale=None):
    from g2o_frontend_amd import api
    pixels = P.rows * P.cols
    collapsed = np.full(W.scene.size() + pixels, -7, np.int32)
    res = api.scene_step(ctx, P.cp, P.ap, P.sp, frame, W.sceneT, W.scene, W.cloud, W.sub, raw_scale=raw_scale, collapsed=collapsed)
    launches = {s: ctx.stage_ms(s)[1] for s in ("project_ref", "project_cur", "corr_linearize", "solve", "scene_render", "scene_pose", "scene_add", "scene_merge")}
    W.sceneT = api._from_colmajor(res.scene_T, 4)
    assert np.all(collapsed[res.size_after_add:] == -1)
    return dict(align=_align_bytes(res.align), T=api._from_colmajor(res.align.T, 4), sceneT=W.sceneT.copy(), n_cloud=res.n_cloud, n_subscene=res.n_subscene,
                size_add=res.size_after_add, size_merge=res.size_after_merge, collapsed=collapsed[:res.size_after_add].copy(), launches=launches)


def same_step(a, b, where):
    for k in ("align", "n_cloud", "n_subscene", "size_add", "size_merge"):
        assert a[k] == b[k], (where, k, a[k] if k != "align" else [f for f in ALIGN_FIELDS if a[k][f] != b[k][f]], b[k] if k != "align" else "")
    assert a["sceneT"].tobytes() == b["sceneT"].tobytes(), (where, a["sceneT"], b["sceneT"])
    assert np.array_equal(a["collapsed"], b["collapsed"]), where


def same_clouds(x, y, where):
    sx, sy = x.snapshot(), y.snapshot()
    assert sorted(sx) == sorted(sy), where
    for k in sx:
        assert sx[k] == sy[k], (where, k)
    assert x.scene.size() == y.scene.size() and x.scene.numGaussians() == y.scene.numGaussians()


def run_both(ctx, P, stream, raw_scale=None, on_device=False, start=None):
    """every frame through both routes on twin clouds, compared after every frame; returns the per-frame results of the one-call route"""
    from g2o_frontend_amd import api
    pixels = P.rows * P.cols
    A, B = Clouds(ctx, pixels), Clouds(ctx, pixels)
    if start is not None:
        A.sceneT, B.sceneT = start.copy(), start.copy()
    out = []
    for k, frame in enumerate(stream):
        f = api.DeviceBuffer(ctx, frame) if on_device else frame
        a = composed(ctx, P, A, f, raw_scale)
        b = one_call(ctx, P, B, f, raw_scale)
        same_step(a, b, k)
        same_clouds(A, B, k)
        out.append(b)
    return out, A, B


@pytest.mark.parametrize("storage", ["sym6", "exact9"])
@pytest.mark.parametrize("offset", [None, OFFSET], ids=["identity", "mounted"])
def test_stream_and_case_h_equal_the_composed_route(contexts, frames, storage, offset):
    ctx = contexts(storage)
    P = Params(ctx, offset)
    steps, _, B = run_both(ctx, P, frames["S"])
    # the first frame meets a scene of size 0: nothing is rendered, the pose stays the identity, the frame is added and merged
    first = steps[0]
    assert first["n_subscene"] == 0 and np.array_equal(first["T"], np.eye(4, dtype=np.float32)) and first["size_add"] == first["n_cloud"] > 10000
    assert steps[S.BLANK]["n_cloud"] == 0 and steps[S.BLANK]["size_add"] == steps[S.BLANK - 1]["size_merge"]
    assert all(s["size_add"] - s["size_merge"] > 10000 for k, s in enumerate(steps) if k not in (0, S.BLANK))
    assert B.scene.numGaussians() == steps[-1]["size_add"] > steps[-1]["size_merge"]            # the Gaussian tail is there
    hsteps, _, _ = run_both(ctx, P, frames["H"])
    h = hsteps[1]
    assert np.array_equal(h["T"], np.eye(4, dtype=np.float32)) and np.array_equal(h["sceneT"], np.eye(4, dtype=np.float32))
    assert h["n_cloud"] > 5000 and h["n_subscene"] > 0 and h["size_add"] == hsteps[0]["size_merge"] + h["n_cloud"]


def test_stream_with_the_convergence_setting(contexts, frames):
    ctx = contexts("sym6")
    ctx.set_convergence(1e-3, 1e-4)
    try:
        P = Params(ctx)
        steps, _, _ = run_both(ctx, P, frames["S"])
        its = [s["align"]["iterations"] for s in steps]
        assert min(its[1:3]) < P.ap.outer_iterations * P.ap.inner_iterations, its      # some pair stopped early
    finally:
        ctx.clear_convergence()


@pytest.mark.parametrize("on_device", [False, True], ids=["host_frames", "device_frames"])
def test_double_size_u16_frames_with_step_2(contexts, frames, on_device):
    ctx = contexts("sym6")
    P = Params(ctx, step=2)
    steps, _, _ = run_both(ctx, P, frames["S2"], raw_scale=0.001, on_device=on_device)
    assert steps[1]["n_cloud"] > 10000 and steps[S.BLANK]["n_cloud"] == 0


def test_a_pose_that_looks_away_from_the_scene(contexts, frames):
    """the sub-scene is empty, the aligner returns the identity, the scene pose stays"""
    ctx = contexts("sym6")
    P = Params(ctx)
    pixels = P.rows * P.cols
    A, B = Clouds(ctx, pixels), Clouds(ctx, pixels)
    for W, step in ((A, composed), (B, one_call)):
        step(ctx, P, W, frames["S"][0])
        W.sceneT = AWAY.copy()
    a, b = composed(ctx, P, A, frames["S"][1]), one_call(ctx, P, B, frames["S"][1])
    same_step(a, b, "away"); same_clouds(A, B, "away")
    assert b["n_subscene"] == 0 and np.array_equal(b["T"], np.eye(4, dtype=np.float32)) and np.array_equal(b["sceneT"], AWAY)


def test_launch_counts(contexts, frames):
    """the alignment's launches are a plain pwn_hip_align's; every new stage is timed once per call"""
    ctx = contexts("sym6")
    ctx.set_profiling(True)
    try:
        P = Params(ctx)
        pixels = P.rows * P.cols
        A, B = Clouds(ctx, pixels), Clouds(ctx, pixels)
        for k in range(2):
            a, b = composed(ctx, P, A, frames["S"][k]), one_call(ctx, P, B, frames["S"][k])
            for s in ("project_ref", "project_cur", "corr_linearize", "solve"):
                assert a["launches"][s] == b["launches"][s], (k, s, a["launches"], b["launches"])
            assert [b["launches"][s] for s in ("scene_render", "scene_pose", "scene_add", "scene_merge")] == [1, 1, 1, 1], (k, b["launches"])
        assert b["launches"]["project_ref"] >= P.ap.outer_iterations - 1
    finally:
        ctx.set_profiling(False)


def test_every_step_repeated_with_the_two_pass_projection(contexts, frames):
    """settle guard 0: a projection gives up on the first pixel two points of it meet in, the step is skipped on the device and repeated with
    k_project_robust, as the composed route's pwn_hip_align is; the bytes are the default path's and the scene does not show the abandoned
    attempt.  Stream W: every step behind the first is repeated.  Stream S: the same bytes too, but only its frame 4 makes two points of a
    reference projection meet (measured, identity and mounted offset alike: repeats 0 0 0 0 1, of pwn_hip_align on the same clouds as well),
    so there the step has to repeat exactly where the composed route's alignment does."""
    ctx = contexts("sym6")
    L = ctx._L
    P = Params(ctx)
    pixels = P.rows * P.cols
    n = C.c_int(0)

    def fallbacks():
        ctx.check(L.pwn_hip_debug_projection_fallbacks(ctx.h, C.byref(n)))
        return n.value
    for name in ("W", "S"):
        A, B, D = Clouds(ctx, pixels), Clouds(ctx, pixels), Clouds(ctx, pixels)
        repeats = []
        try:
            for k, frame in enumerate(frames[name]):
                a = one_call(ctx, P, A, frame)
                ctx.check(L.pwn_hip_debug_set_settle_guard(ctx.h, 0))
                n0 = fallbacks(); b = one_call(ctx, P, B, frame)
                n1 = fallbacks(); d = composed(ctx, P, D, frame)
                n2 = fallbacks()
                ctx.check(L.pwn_hip_debug_set_settle_guard(ctx.h, -1))
                repeats.append((n1 - n0, n2 - n1))
                print("stream", name, "frame", k, "repeats of the one-call step and of the composed route's alignment:", repeats[-1])
                same_step(a, b, (name, k)); same_clouds(A, B, (name, k))
                same_step(a, d, (name, k)); same_clouds(A, D, (name, k))
        finally:
            ctx.check(L.pwn_hip_debug_set_settle_guard(ctx.h, -1))
        assert all(x == y for x, y in repeats), (name, repeats)
        if name == "W":
            assert [x for x, _ in repeats] == [0, 1, 1], repeats      # the first frame has no reference to project
        else:
            assert repeats[4] == (1, 1), repeats


def test_refusals_leave_the_clouds_alone(contexts, frames):
    from g2o_frontend_amd import api
    ctx = contexts("sym6")
    P = Params(ctx)
    pixels = P.rows * P.cols
    W = Clouds(ctx, pixels)
    one_call(ctx, P, W, frames["S"][0])
    one_call(ctx, P, W, frames["S"][1])
    before = W.snapshot()

    def refused(code, scene, cloud, sub):
        with pytest.raises(api.PwnHipError) as e:
            api.scene_step(ctx, P.cp, P.ap, P.sp, frames["S"][2], W.sceneT, scene, cloud, sub)
        assert e.value.code == code, e.value
        assert W.snapshot() == before
    # capacity one point short of size + rows * cols
    tight = api.Cloud(ctx, W.scene.size() + pixels - 1)
    tight.add(W.scene)
    assert tight.size() == W.scene.size() and tight.numGaussians() >= tight.size()
    tb = tight.arrays(stats=True)
    refused(6, tight, W.cloud, W.sub)
    assert all(np.array_equal(v, tight.arrays(stats=True)[k]) for k, v in tb.items())
    # a scene with fewer Gaussians than points
    bare = api.Cloud(ctx, 4 * pixels)
    a = W.scene.arrays()
    bare.upload(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])
    refused(1, bare, W.cloud, W.sub)
    assert bare.size() == W.scene.size() and bare.numGaussians() == 0
    # equal handles
    refused(1, W.scene, W.cloud, W.cloud)
    refused(1, W.scene, W.scene, W.sub)
    # and the step still runs
    assert one_call(ctx, P, W, frames["S"][2])["n_cloud"] > 10000


def test_scene_aligner_equals_the_raw_calls(contexts, frames):
    from g2o_frontend_amd import api
    ctx = contexts("sym6")
    P = Params(ctx)
    pixels = P.rows * P.cols
    W = Clouds(ctx, pixels)
    Q = Params(ctx)
    sa = api.SceneAligner(ctx, Q.converter, Q.aligner, Q.merger, (S.N_FRAMES + 1) * pixels)
    G = np.eye(4, dtype=np.float32)
    for k, frame in enumerate(frames["S"]):
        r = one_call(ctx, P, W, frame)
        T = sa.processFrame(frame)
        assert T.tobytes() == r["T"].tobytes() and sa.sceneT().tobytes() == r["sceneT"].tobytes(), k
        assert np.array_equal(sa.collapsedIndices(), r["collapsed"])
        G = _mul(ctx._L, G, r["T"]); G[3] = (0, 0, 0, 1)
        assert sa.globalT().tobytes() == G.tobytes()
        same_clouds(W, Clouds.of(sa.scene(), sa.cloud(), sa.subscene()), k)
    old = sa.newChunk()
    assert old.size() == W.scene.size() and sa.scene().size() > 0 and np.array_equal(sa.sceneT(), np.eye(4, dtype=np.float32))
