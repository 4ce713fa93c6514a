"""A cloud's device arrays over its lifetime: a cloud with a history -- a scene with Stats, explicit normal information, Gaussians and the second
array set of the compactions; a cloud out of the context's pool -- against a freshly created cloud given the same final content, every
downloadable array bit for bit (points, normals, curvature, both information matrices, Stats where present, the Gaussians and their flags, the
size).  24 x 32 frames of the synthetic scene, clouds of 4 x 768 points.  The calls that replace a cloud's content -- conversions, upload, unProject,
import, load, the pool -- leave nothing of the history behind, a conversion that fails leaves an empty cloud, a refused one an untouched cloud."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_clouds as S      # noqa: E402
from test_gpu_scene_clouds import same_snapshot      # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
ROWS, COLS = 24, 32
CAP = 4 * ROWS * COLS
RES = 0.05
CONF = dict(S.CONVERTER_CONF, world_radius=0.25)      # fx = 26.25: a window of about 3 pixels at 2 m, inside [min, max]_image_radius
T_MOVE = (S.isometry((0.04, -0.02, 0.03, 0.01, -0.02, 0.015)), S.isometry((-0.03, 0.05, 0.01, -0.015, 0.01, 0.02)))


def k_small():
    from g2o_frontend_amd import synth
    return synth.scaled_K(synth.K_VGA, 20)


@pytest.fixture(scope="module")
def frames():
    from g2o_frontend_amd import synth
    out = []
    for seed in (1, 2):
        ref, cur, _ = synth.make_pair(seed, ROWS, COLS, k_small())
        out += [ref.astype(F) * F(0.001), cur.astype(F) * F(0.001)]
    return out


@pytest.fixture(scope="module")
def ctx():
    from g2o_frontend_amd import api
    c = api.Context(device=0, max_rows=S.ROWS, max_cols=S.COLS, max_batch=1)      # the injected clouds of scene_clouds are 48 x 64
    yield c
    c.close()


def projector(api):
    K = k_small()
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    proj.setMinDistance(CONF["min_distance"]); proj.setMaxDistance(CONF["max_distance"]); proj.setImageSize(ROWS, COLS)
    return proj


def make_converter(api):
    st = api.StatsCalculatorIntegralImage()
    st.setWorldRadius(CONF["world_radius"]); st.setMinImageRadius(CONF["min_image_radius"]); st.setMaxImageRadius(CONF["max_image_radius"])
    st.setMinPoints(CONF["min_points"]); st.setCurvatureThreshold(CONF["stats_curvature_threshold"])
    pi, ni = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
    pi.setCurvatureThreshold(CONF["point_info_curvature_threshold"]); ni.setCurvatureThreshold(CONF["normal_info_curvature_threshold"])
    return api.DepthImageConverterIntegralImage(projector(api), st, pi, ni)


def converted(context, frame, capacity=ROWS * COLS, keep_stats=False, gaussians=False):
    from g2o_frontend_amd import api
    c = api.Cloud(context, capacity)
    make_converter(api).compute(c, frame, keep_stats=keep_stats, gaussians=gaussians)
    return c


def destroy(c):
    c.ctx.check(c.ctx._L.pwn_hip_cloud_destroy(c.ctx.h, c.h))
    c.h = None


def snapshot(c):
    from g2o_frontend_amd._lib import PwnHipError
    try:
        a = c.arrays(stats=True)
    except PwnHipError as e:
        assert "not converted with keep_stats" in str(e)
        a = c.arrays()
    a["gauss"] = c.gaussians()
    a["size"] = c.size()
    return a


def assert_same(a, b, what):
    assert a["size"] == b["size"] and sorted(a) == sorted(b), (what, a["size"], b["size"], sorted(a), sorted(b))
    for k in a:
        if k == "gauss":
            for q in S.GAUSS_KEYS:
                assert a[k][q].tobytes() == b[k][q].tobytes(), (what, "gauss", q)
        elif k != "size":
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


def scene(context, frames):
    """view 0 and view 1 with Stats and Gaussians added into one cloud, merged and voxelized: explicit normal information, Stats, Gaussians and
    the second array set with all of them"""
    from g2o_frontend_amd import api
    sc = api.Cloud(context, CAP)
    for f, T in zip(frames[:2], (S.EYE, T_MOVE[0])):
        sc.add(converted(context, f, keep_stats=True, gaussians=True), T)
    m = api.Merger(); m.setImageSize(ROWS, COLS); m.setMaxPointDepth(4.0)
    m.setDepthImageConverter(api.DepthImageConverterIntegralImage(projector(api), None, None, None))
    n = sc.size()
    k = m.merge(sc, S.EYE)
    assert 0 < k < n and sc.numGaussians() == n
    assert 0 < api.VoxelCalculator().compute(sc, RES) <= k
    return sc


def uploaded(context, capacity=CAP, n=None):
    """an uploaded cloud -- explicit normal information -- with a Gaussian for every point"""
    from g2o_frontend_amd import api
    src = S.add_source()
    n = src["n"] if n is None else n
    c = api.Cloud(context, capacity)
    c.upload(*[src["arrays"][k][:n] for k in S.CLOUD_KEYS])
    c.debugSetGaussians(*[S.head_gauss(src["gauss"], n)[k] for k in S.GAUSS_KEYS])
    assert c.size() == c.numGaussians() == n and c.arrays()["omega_n"].any()
    return c


def make_aligner(context):
    """the converter's projector, so that the aligner's index key is the converted clouds' and the projection shortcuts are taken"""
    from g2o_frontend_amd import api
    finder = api.CorrespondenceFinder(); finder.setImageSize(ROWS, COLS)
    a = api.Aligner(context)
    a.setProjector(projector(api)); a.setLinearizer(api.Linearizer()); a.setCorrespondenceFinder(finder)
    a.setOuterIterations(3); a.setInnerIterations(1)
    return a


def aligned(aligner, ref, cur):
    aligner.setReferenceCloud(ref); aligner.setCurrentCloud(cur)
    r = aligner.align()
    assert r["iterations"] == 3 and r["inliers"] > 0
    return [r[k].tobytes() for k in ("T", "chi2", "iter_inliers", "C", "K")] + [r["n_reference"], r["n_current"]]


@pytest.mark.parametrize("how", ["plain", "keep_stats", "gaussians"])
def test_compute_over_a_used_cloud(ctx, frames, how):
    """a conversion replaces whatever the cloud held, and the index image it promises while it is queued is the new content's: the cloud equals a
    fresh one, and aligns like it on either side of a pair"""
    from g2o_frontend_amd import api
    other = converted(ctx, frames[1])
    aligner = make_aligner(ctx)
    got = []
    for c in (scene(ctx, frames), api.Cloud(ctx, CAP)):
        make_converter(api).compute(c, frames[0], keep_stats=how == "keep_stats", gaussians=how == "gaussians")
        got.append((snapshot(c), aligned(aligner, other, c), aligned(aligner, c, other)))
    assert_same(got[0][0], got[1][0], how)
    assert ("stats" in got[0][0]) == (how == "keep_stats") and len(got[0][0]["gauss"]["flags"]) == (got[0][0]["size"] if how == "gaussians" else 0)
    assert got[0][1:] == got[1][1:], how


@pytest.fixture(scope="module")
def ctx2():
    from g2o_frontend_amd import api
    c = api.Context(device=0, max_rows=S.ROWS, max_cols=S.COLS, max_batch=2)
    yield c
    c.close()


@pytest.mark.parametrize("form", ["batch", "scaled"])
def test_batch_forms_over_used_clouds(ctx2, frames, form):
    """computeBatch of two frames, and the 2 x scaled batch form from 48 x 64 sources, over a scene and over an uploaded cloud with Gaussians"""
    import ctypes as C
    from g2o_frontend_amd import api, synth
    conv = make_converter(api)
    if form == "scaled":
        src = [synth.make_pair(seed, 2 * ROWS, 2 * COLS, synth.scaled_K(synth.K_VGA, 10))[0].astype(F) * F(0.001) for seed in (3, 4)]
        ptrs, p = (C.c_void_p * 2)(*[f.ctypes.data for f in src]), conv.params()
    snaps = []
    for clouds in ((scene(ctx2, frames), uploaded(ctx2)), (api.Cloud(ctx2, CAP), api.Cloud(ctx2, CAP))):
        if form == "batch":
            conv.computeBatch(list(clouds), frames[2:4])
        else:
            handles = (C.c_void_p * 2)(*[c.h for c in clouds])
            ctx2.check(ctx2._L.pwn_hip_convert_batch_scaled(ctx2.h, C.byref(p), ptrs, 2, 2 * ROWS, 2 * COLS, 2, 0.01, handles))
        snaps.append([snapshot(c) for c in clouds])
    for i, (a, b) in enumerate(zip(*snaps)):
        assert a["size"] > ROWS * COLS // 2 and a["normals"].any()
        assert_same(a, b, (form, i))


def test_upload_over_a_cloud_with_gaussians(ctx):
    """the Gaussians belonged to the points that are gone"""
    from g2o_frontend_amd import api
    src = S.add_source(seed=22)
    snaps = []
    for c in (uploaded(ctx), api.Cloud(ctx, CAP)):
        c.upload(*[src["arrays"][k] for k in S.CLOUD_KEYS])
        assert c.numGaussians() == 0
        snaps.append(snapshot(c))
    assert_same(snaps[0], snaps[1], "upload")


def test_unproject_over_an_uploaded_cloud_with_gaussians(ctx, frames):
    """points only: zero normals, and zero normal information for them, not the rows the uploaded points left behind"""
    from g2o_frontend_amd import api
    snaps = []
    for c in (uploaded(ctx), api.Cloud(ctx, CAP)):
        projector(api).unProject(c, frames[0])
        snaps.append(snapshot(c))
    assert snaps[0]["size"] > ROWS * COLS // 2 and not snaps[1]["omega_n"].any() and not snaps[1]["normals"].any()
    assert len(snaps[1]["gauss"]["flags"]) == 0
    assert_same(snaps[0], snaps[1], "unProject")


def test_a_refused_batch_leaves_its_first_cloud_as_it_was(ctx2, frames):
    import ctypes as C
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import PwnHipError
    first, second = uploaded(ctx2), api.Cloud(ctx2, CAP)
    before = snapshot(first)
    p = make_converter(api).params()
    ptrs, handles = (C.c_void_p * 2)(frames[2].ctypes.data, None), (C.c_void_p * 2)(first.h, second.h)
    with pytest.raises(PwnHipError, match="null frame or cloud"):
        ctx2.check(ctx2._L.pwn_hip_convert_batch(ctx2.h, C.byref(p), ptrs, 2, ROWS, COLS, handles))
    assert_same(snapshot(first), before, "refused batch")
    assert before["size"] > 0 and len(before["gauss"]["flags"]) == before["size"]


def test_a_conversion_that_fails_leaves_an_empty_cloud(ctx):
    """PWN_HIP_ERR_CAPACITY: 768 valid pixels into a cloud of 16 points (the kernels' stores are guarded by the capacity; the call returns the
    status when it has seen the count).  The cloud must not go on reporting the 16 uploaded points and their Gaussians over arrays the failed
    conversion wrote into."""
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import PwnHipError, STATUS
    c = uploaded(ctx, capacity=16, n=16)
    with pytest.raises(PwnHipError) as e:
        make_converter(api).compute(c, np.full((ROWS, COLS), 2.0, F), keep_stats=True)
    assert STATUS[e.value.code] == "CAPACITY"
    assert c.size() == 0 and c.numGaussians() == 0
    with pytest.raises(PwnHipError, match="not converted with keep_stats"):
        c.arrays(stats=True)
    small = (np.arange(16, dtype=F).reshape(4, 4) * F(0.01) + F(2.0))
    fresh = api.Cloud(ctx, 16)
    for x in (c, fresh):
        make_converter(api).compute(x, small)
    assert fresh.size() == 16
    assert_same(snapshot(c), snapshot(fresh), "after a failed conversion")


def test_back_set_survives_an_import_of_a_class_coded_cloud(ctx, frames):
    """A scene cloud's second array set keeps its explicit normal information when an import of a class-coded cloud drops the front's: the next
    compaction must not bring it back.  Once as import, add, voxelize; once with the voxelize right behind the import."""
    from g2o_frontend_amd import api
    plain = converted(ctx, frames[2])
    flat = np.zeros(plain.flatSize(), np.uint8)
    assert plain.exportFlat(flat) == flat.size
    want_n = plain.arrays()["omega_n"]
    assert want_n.any() and len(want_n) > ROWS * COLS // 2
    late = converted(ctx, frames[3], keep_stats=True, gaussians=True)
    vox = api.VoxelCalculator()
    for with_add in (True, False):
        clouds = scene(ctx, frames), api.Cloud(ctx, CAP)
        snaps = []
        for c in clouds:
            c.importFlat(flat)
            steps = [snapshot(c)]
            if with_add:
                c.add(late, T_MOVE[1])
                steps.append(snapshot(c))
            assert vox.compute(c, RES) > 0
            steps.append(snapshot(c))
            snaps.append(steps)
        for step, (a, b) in enumerate(zip(*snaps)):
            assert_same(a, b, ("with add" if with_add else "without add", step))
        assert snaps[0][0]["omega_n"].tobytes() == want_n.tobytes()
        if not with_add:      # no transform since the import: the class matrices of the imported cloud, gathered
            kept = vox.keptIndices()
            assert snaps[0][-1]["omega_n"].tobytes() == want_n[kept].tobytes()


def test_a_pooled_cloud_is_a_new_cloud(ctx, frames):
    from g2o_frontend_amd import api
    first = converted(ctx, frames[0])
    assert first.size() > 0
    destroy(first)
    again = converted(ctx, frames[1])                 # same capacity: out of the pool
    other = api.Context(device=0, max_rows=ROWS, max_cols=COLS, max_batch=1)
    try:
        fresh = converted(other, frames[1])
        assert_same(snapshot(again), snapshot(fresh), "pool reuse")
        del fresh
    finally:
        other.close()


def test_a_scene_cloud_does_not_retire_into_the_pool(ctx, frames):
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import PwnHipError
    sc = scene(ctx, frames)
    # (the voxelization has emptied the Gaussian vector, voxelcalculator.cpp:62-64; the cloud still holds the arrays)
    assert sc.arrays(stats=True)["stats"].shape == (sc.size(), 16)
    destroy(sc)
    c = api.Cloud(ctx, CAP)
    assert c.size() == 0 and c.numGaussians() == 0
    with pytest.raises(PwnHipError, match="not converted with keep_stats"):
        c.arrays(stats=True)


def test_both_omega_storages_in_one_context(ctx, oracle):
    """a cloud created under exact9 and one under sym6, each through Cloud::add (a moved cloud, then one whose points merge) and Merger::merge,
    against the oracle.  The matrices that go in are exactly symmetric and the result of one add is compared, so sym6's stored upper triangle
    is the oracle's in every bit."""
    orc = S.OracleSide(oracle)
    src, case = S.add_source(), S.flags_case()
    try:
        for storage in ("exact9", "sym6"):
            ctx.set_omega_storage(storage)
            dev = S.DeviceSide(ctx)
            got = []
            for side in (orc, dev):
                dst = side.empty(CAP)
                side.add(dst, side.cloud(src["arrays"], src["gauss"]), S.T_A)
                side.add(dst, side.cloud(case["arrays"], case["gauss"]), S.EYE)
                k, col = side.merge(dst, case["cfg"])
                got.append((k, col, side.snapshot(dst)))
            assert dev.empty(1).omega_storage() == storage
            assert got[0][0] == got[1][0] < src["n"] + case["n"] and np.array_equal(got[0][1], got[1][1])
            same_snapshot(got[0][2], got[1][2], storage, sym6=storage == "sym6")
    finally:
        ctx.set_omega_storage(type(ctx).DEFAULT_OMEGA_STORAGE)


def test_load_over_a_scene(ctx, frames, tmp_path):
    from g2o_frontend_amd import api
    path = tmp_path / "cloud.pwn"
    converted(ctx, frames[2], keep_stats=True).save(path, T_MOVE[1], binary=True)
    snaps = []
    for c in (scene(ctx, frames), api.Cloud(ctx, CAP)):
        T = c.load(path)
        steps = [snapshot(c)]
        assert steps[0]["size"] > ROWS * COLS // 2 and np.array_equal(T, snaps[0][2] if snaps else T)
        assert api.VoxelCalculator().compute(c, RES) > 0
        steps += [snapshot(c), T]
        snaps.append(steps)
    for step in (0, 1):
        assert_same(snaps[0][step], snaps[1][step], ("load", step))
