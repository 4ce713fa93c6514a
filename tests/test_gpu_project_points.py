"""PinholePointProjector::project on the GPU, every launch form on the injected points of tests/project_points.py: the stand-alone projection
(pwn_hip_project), the aligner's latency (k_project<1>), throughput (k_project<4>) and two-pass (k_project_robust) launches through
pwn_hip_debug_project_pairs, and the depth-only batch (pwn_hip_project_merge_batch).  Every comparison is of words: index images, and depth
images viewed as uint32, against the oracle's (for the `far` case, which the oracle is not asked: against the empty images).  One context for
the whole module, never cleared: every launch finds what the launches before it left in the z-buffers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_points as PP      # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, CAPACITY = 1, 6


@pytest.fixture(scope="module")
def ctx():
    from g2o_frontend_amd import api
    c = api.Context(device=0, max_rows=64, max_cols=64, max_batch=16, omega_storage="exact9")
    c._pp_clouds = {}
    yield c
    c._pp_clouds.clear()
    c.close()


@pytest.fixture(scope="module")
def cases(oracle):
    return PP.all_cases()


@pytest.fixture(scope="module")
def want(cases, oracle):
    """the oracle's images per case, computed once"""
    out = {}
    for c in cases:
        out[c.name] = oracle.project(c.K, c.T, c.min_d, c.max_d, c.rows, c.cols, c.points4()) if c.ask_oracle else PP.empty_images(c)
    return out


def upload(ctx, cloud, P):
    """points only: normals, curvature and information matrices zero (the projection reads none of them); n = 0 is an upload like any other"""
    n = len(P)
    m = max(1, n)
    p4 = np.zeros((m, 4), F); p4[:n, :3] = P; p4[:, 3] = 1.0
    z4, z1, z16 = np.zeros((m, 4), F), np.zeros(m, F), np.zeros((m, 16), F)
    ctx.check(ctx._L.pwn_hip_cloud_upload(ctx.h, cloud.h, n, p4.ctypes.data, z4.ctypes.data, z1.ctypes.data, z16.ctypes.data, z16.ctypes.data))


def cloud_of(ctx, case, roomy=False):
    """the case's device cloud: capacity = its size, or (roomy) PP.SIZES_CAPACITY with landing points behind the case's own"""
    from g2o_frontend_amd import api
    key = (case.name, roomy)
    if key not in ctx._pp_clouds:
        c = api.Cloud(ctx, PP.SIZES_CAPACITY if roomy else max(1, case.n))
        if roomy:
            upload(ctx, c, PP.stale_points(case))
        upload(ctx, c, case.P)
        assert c.size() == case.n
        ctx._pp_clouds[key] = c
    return ctx._pp_clouds[key]


def aligner_params(case):
    from g2o_frontend_amd import _lib, api
    p = _lib.AlignerParams()
    _lib.lib().pwn_hip_default_aligner_params(C.byref(p))
    api._set(p.K, np.array([[case.K[0], 0, case.K[2]], [0, case.K[1], case.K[3]], [0, 0, 1]], F), 3)
    p.min_distance, p.max_distance, p.rows, p.cols = case.min_d, case.max_d, case.rows, case.cols
    return p


def colmajor(Ts):
    return np.ascontiguousarray(np.stack([np.asarray(T, F).T.reshape(-1) for T in Ts]), F)


def project_pairs(ctx, batch, which, form, clouds=None, transforms=None, check=True):
    """pwn_hip_debug_project_pairs on the cases of `batch` (one image, camera and range) -> (index [n, rows, cols], depth, gave_up)"""
    c0 = batch[0]
    n = len(batch)
    clouds = clouds if clouds is not None else [cloud_of(ctx, c) for c in batch]
    handles = (C.c_void_p * n)(*[c.h for c in clouds])
    tr = colmajor(transforms if transforms is not None else [c.T for c in batch])
    idx = np.full((n, c0.rows, c0.cols), -9, np.int32); dep = np.full((n, c0.rows, c0.cols), -9, F)
    g = C.c_int(-9)
    p = aligner_params(c0)
    rc = ctx._L.pwn_hip_debug_project_pairs(ctx.h, C.byref(p), n, handles, tr.ctypes.data, which, form, idx.ctypes.data, dep.ctypes.data, C.byref(g))
    if check:
        ctx.check(rc)
    return idx, dep, g.value


def stand_alone(ctx, case, cloud=None):
    from g2o_frontend_amd import api
    pr = api.PinholePointProjector(ctx)
    pr.setCameraMatrix([[case.K[0], 0, case.K[2]], [0, case.K[1], case.K[3]], [0, 0, 1]]); pr.setTransform(case.T)
    pr.setMinDistance(case.min_d); pr.setMaxDistance(case.max_d); pr.setImageSize(case.rows, case.cols)
    return pr.project(cloud if cloud is not None else cloud_of(ctx, case))


def depth_planes(ctx, batch, clouds=None):
    """pwn_hip_project_merge_batch's planes, merged and weights zeroed"""
    c0 = batch[0]
    n = len(batch)
    clouds = clouds if clouds is not None else [cloud_of(ctx, c) for c in batch]
    handles = (C.c_void_p * n)(*[c.h for c in clouds])
    Kc = np.array([c0.K[0], 0, 0, 0, c0.K[1], 0, c0.K[2], c0.K[3], 1], F)
    tr = colmajor([c.T for c in batch])
    out, w = np.zeros((c0.rows, c0.cols), F), np.zeros((c0.rows, c0.cols), F)
    planes = np.full((n, c0.rows, c0.cols), -9, F)
    ctx.check(ctx._L.pwn_hip_project_merge_batch(ctx.h, Kc.ctypes.data, n, handles, tr.ctypes.data, c0.min_d, c0.max_d, c0.rows, c0.cols, out.ctypes.data,
                                                 w.ctypes.data, None, None, planes.ctypes.data))
    return planes


def same(case, got_index, got_depth, want, what):
    wi, wd = want[case.name]
    ok = (got_index is None or np.array_equal(got_index, wi)) and np.array_equal(PP.bits(got_depth), PP.bits(wd))
    assert ok, f"{what}: " + PP.describe_difference(case, wi if got_index is None else got_index, got_depth, wi, wd)


# ------------------------------------------------------------------------------------------------- 1. every form against the oracle
def test_stand_alone_projection_on_every_case(ctx, cases, want):
    for c in cases:
        idx, dep = stand_alone(ctx, c)
        same(c, idx, dep, want, "pwn_hip_project")


@pytest.mark.parametrize("which", [0, 1])
def test_latency_launch_on_every_case(ctx, cases, want, which):
    for c in cases:
        idx, dep, gave_up = project_pairs(ctx, [c], which, 0)
        assert gave_up == 0, c.name
        same(c, idx[0], dep[0], want, f"k_project<1>, which = {which}")


@pytest.mark.parametrize("which", [0, 1])
def test_throughput_launch_on_every_case(ctx, cases, want, which):
    for batch in PP.batches(cases):
        idx, dep, gave_up = project_pairs(ctx, batch, which, 0)
        assert gave_up == 0, [c.name for c in batch]
        for i, c in enumerate(batch):
            same(c, idx[i], dep[i], want, f"k_project<4>, which = {which}, pair {i}")


@pytest.mark.parametrize("which", [0, 1])
def test_two_pass_launch_on_every_case(ctx, cases, want, which):
    for c in cases:
        idx, dep, gave_up = project_pairs(ctx, [c], which, 1)
        assert gave_up == 0, c.name
        same(c, idx[0], dep[0], want, f"k_project_robust, one pair, which = {which}")
    for batch in PP.batches(cases):
        idx, dep, gave_up = project_pairs(ctx, batch, which, 1)
        assert gave_up == 0
        for i, c in enumerate(batch):
            same(c, idx[i], dep[i], want, f"k_project_robust, which = {which}, pair {i}")


def test_depth_only_batch_on_every_case(ctx, cases, want):
    for c in cases:
        same(c, None, depth_planes(ctx, [c])[0], want, "k_project_depth_batch, one cloud")
    for batch in PP.batches(cases):
        planes = depth_planes(ctx, batch)
        for i, c in enumerate(batch):
            same(c, None, planes[i], want, f"k_project_depth_batch, cloud {i} of nine")


@pytest.mark.parametrize("which", [0, 1])
def test_clouds_with_room_behind_their_points(ctx, cases, want, which):
    """the nine sizes in clouds of capacity 3072 whose arrays hold nearer points of an earlier upload behind the cloud's size: the grid is sized by
    the capacity, the count decides what is read"""
    batch = [c for c in cases if c.name.startswith("sizes")]
    clouds = [cloud_of(ctx, c, roomy=True) for c in batch]
    for form in (0, 1):
        idx, dep, gave_up = project_pairs(ctx, batch, which, form, clouds=clouds)
        assert gave_up == 0
        for i, c in enumerate(batch):
            same(c, idx[i], dep[i], want, f"capacity 3072, nine pairs, form {form}, which = {which}")
            i1, d1, g1 = project_pairs(ctx, [c], which, form, clouds=[clouds[i]])
            assert g1 == 0
            same(c, i1[0], d1[0], want, f"capacity 3072, one pair, form {form}, which = {which}")
    if which == 0:
        planes = depth_planes(ctx, batch, clouds=clouds)
        for i, c in enumerate(batch):
            same(c, None, planes[i], want, "capacity 3072, depth only")
            same(c, *stand_alone(ctx, c, clouds[i]), want, "capacity 3072, pwn_hip_project")


# ------------------------------------------------------------------------------------------------- 2. the forms agree with each other
def test_forms_agree_on_the_nine_pair_launch(ctx, cases):
    batch = [c for c in cases if c.name.startswith("sizes")]
    for which in (0, 1):
        ti, td, _ = project_pairs(ctx, batch, which, 0)
        ri, rd, _ = project_pairs(ctx, batch, which, 1)
        assert np.array_equal(ti, ri) and np.array_equal(PP.bits(td), PP.bits(rd))
        for i, c in enumerate(batch):
            li, ld, _ = project_pairs(ctx, [c], which, 0)
            assert np.array_equal(li[0], ti[i]) and np.array_equal(PP.bits(ld[0]), PP.bits(td[i])), PP.describe_difference(c, li[0], ld[0], ti[i], td[i])


# ------------------------------------------------------------------------------------------------- 3. nothing stale
def test_nothing_stale_between_projections(ctx, cases, want):
    """A fills every pixel, B a few of them, C has the other image size (another word layout over the same slots), then A again -- in one
    context, nothing cleared in between: the images are the oracle's for that case alone"""
    A, B, C_ = PP.case_named("sizes/wide/1025"), PP.case_named("round_tie/wide/col1"), PP.case_named("round_tie/tele/col0")
    assert int((want[A.name][0] >= 0).sum()) == A.rows * A.cols and int((want[B.name][0] >= 0).sum()) < 64
    for c in (A, B, C_, A):
        same(c, *stand_alone(ctx, c), want, "pwn_hip_project after another case")
    for which in (0, 1):
        for form in (0, 1):
            for c in (A, B, C_, A):
                idx, dep, _ = project_pairs(ctx, [c], which, form)
                same(c, idx[0], dep[0], want, f"one pair after another case, form {form}, which = {which}")
    bs = PP.batches(cases)
    of = lambda c: next(b for b in bs if any(x is c for x in b))      # noqa: E731
    for batch in (of(A), of(B), of(C_), of(A)):
        idx, dep, _ = project_pairs(ctx, batch, 0, 0)
        for i, c in enumerate(batch):
            same(c, idx[i], dep[i], want, "nine pairs after another launch")


# ------------------------------------------------------------------------------------------------- 4. the hook is the shipped path
@pytest.mark.parametrize("name,other", [("round_tie/wide/small/col", "round_tie/wide/col0"), ("collide/wide", "depth_edge/wide/0.5-5/identity")])
def test_an_alignment_leaves_the_words_the_hook_returns(ctx, want, name, other):
    """Aligner.align with one outer and one inner iteration and the case's transform as the guess: the finder's reference images are the words
    pwn_hip_debug_project_pairs(which = 0) returns for the reference cloud, its current images those of which = 1 under the identity"""
    from g2o_frontend_amd import api
    ref, cur = PP.case_named(name), PP.case_named(other)
    pr = api.PinholePointProjector(ctx)
    pr.setCameraMatrix([[ref.K[0], 0, ref.K[2]], [0, ref.K[1], ref.K[3]], [0, 0, 1]])
    pr.setMinDistance(ref.min_d); pr.setMaxDistance(ref.max_d); pr.setImageSize(ref.rows, ref.cols)
    finder = api.CorrespondenceFinder(); finder.setImageSize(ref.rows, ref.cols)
    al = api.Aligner(ctx)
    al.setProjector(pr); al.setLinearizer(api.Linearizer()); al.setCorrespondenceFinder(finder)
    al.setReferenceCloud(cloud_of(ctx, ref)); al.setCurrentCloud(cloud_of(ctx, cur))
    al.setOuterIterations(1); al.setInnerIterations(1); al.setInitialGuess(ref.T)
    ctx.check(ctx._L.pwn_hip_debug_set_index_shortcut(ctx.h, 0))
    try:
        al.align(images=True)
    finally:
        ctx.check(ctx._L.pwn_hip_debug_set_index_shortcut(ctx.h, 1))
    ri, rd, g = project_pairs(ctx, [ref], 0, 0)
    assert g == 0
    ci, cd, g = project_pairs(ctx, [ref], 1, 0, clouds=[cloud_of(ctx, cur)], transforms=[np.eye(4, dtype=F)])
    assert g == 0
    assert np.array_equal(finder.referenceIndexImage(), ri[0]) and np.array_equal(PP.bits(finder.referenceDepthImage()), PP.bits(rd[0])), \
        PP.describe_difference(ref, finder.referenceIndexImage(), finder.referenceDepthImage(), ri[0], rd[0])
    assert np.array_equal(finder.currentIndexImage(), ci[0]) and np.array_equal(PP.bits(finder.currentDepthImage()), PP.bits(cd[0]))
    same(ref, ri[0], rd[0], want, "the reference side")
    assert (ci[0] >= 0).any()


# ------------------------------------------------------------------------------------------------- 5. a give-up is reported
def test_give_up_is_reported_never_silent(ctx, cases, want):
    col, plain = PP.case_named("collide/wide"), PP.case_named("sizes/wide/257")
    assert int((want[plain.name][0] >= 0).sum()) == plain.n      # one point per pixel: no collision
    ctx.check(ctx._L.pwn_hip_debug_set_settle_guard(ctx.h, 0))
    try:
        for which in (0, 1):
            _, _, g = project_pairs(ctx, [col], which, 0)
            assert g == 1
            batch = next(b for b in PP.batches(cases) if any(x is col for x in b))
            _, _, g = project_pairs(ctx, batch, which, 0)
            assert g == 1
            idx, dep, g = project_pairs(ctx, [col], which, 1)
            assert g == 0
            same(col, idx[0], dep[0], want, "two-pass under guard 0")
            idx, dep, g = project_pairs(ctx, [plain], which, 0)
            assert g == 0
            same(plain, idx[0], dep[0], want, "no collision under guard 0")
    finally:
        ctx.check(ctx._L.pwn_hip_debug_set_settle_guard(ctx.h, -1))
    idx, dep, g = project_pairs(ctx, [col], 0, 0)
    assert g == 0
    same(col, idx[0], dep[0], want, "the default guard again")


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_outputs_alone(ctx, cases):
    """every refusal of include/pwn_hip_testing.h; afterwards the outputs and *gave_up, pre-filled with a sentinel, are as they were"""
    from g2o_frontend_amd import api
    c = PP.case_named("round_tie/wide/col1")
    cloud = cloud_of(ctx, c)
    L = ctx._L
    N = c.rows * c.cols
    idx = np.full(17 * N, -9, np.int32); dep = np.full(17 * N, -9, F)
    g = C.c_int(-9)
    one = (C.c_void_p * 1)(cloud.h)
    many = (C.c_void_p * 17)(*([cloud.h] * 17))
    null_cloud = (C.c_void_p * 1)(None)
    tr = colmajor([c.T] * 17)
    p = aligner_params(c)
    neg = aligner_params(c); neg.min_distance = -0.1
    tall = aligner_params(c); tall.rows = 65
    big = aligner_params(c); big.rows, big.cols = 64, 64 + 1
    zero = aligner_params(c); zero.rows = 0
    other = api.Context(device=0, max_rows=8, max_cols=8, max_batch=1)
    try:
        foreign = api.Cloud(other, 4)
        theirs = (C.c_void_p * 1)(foreign.h)
        P, T, I, D, G = C.byref(p), tr.ctypes.data, idx.ctypes.data, dep.ctypes.data, C.byref(g)
        refused = [
            ("null p", INVALID, (ctx.h, None, 1, one, T, 0, 0, I, D, G)),
            ("null clouds", INVALID, (ctx.h, P, 1, None, T, 0, 0, I, D, G)),
            ("null transforms", INVALID, (ctx.h, P, 1, one, None, 0, 0, I, D, G)),
            ("null gave_up", INVALID, (ctx.h, P, 1, one, T, 0, 0, I, D, None)),
            ("null cloud", INVALID, (ctx.h, P, 1, null_cloud, T, 0, 0, I, D, G)),
            ("n = 0", INVALID, (ctx.h, P, 0, one, T, 0, 0, I, D, G)),
            ("n > max_batch", INVALID, (ctx.h, P, 17, many, T, 0, 0, I, D, G)),
            ("which = 2", INVALID, (ctx.h, P, 1, one, T, 2, 0, I, D, G)),
            ("which = -1", INVALID, (ctx.h, P, 1, one, T, -1, 0, I, D, G)),
            ("form = 2", INVALID, (ctx.h, P, 1, one, T, 0, 2, I, D, G)),
            ("min_distance < 0", INVALID, (ctx.h, C.byref(neg), 1, one, T, 0, 0, I, D, G)),
            ("another context's cloud", INVALID, (ctx.h, P, 1, theirs, T, 0, 0, I, D, G)),
            ("65 rows", CAPACITY, (ctx.h, C.byref(tall), 1, one, T, 0, 0, I, D, G)),
            ("64 x 65", CAPACITY, (ctx.h, C.byref(big), 1, one, T, 0, 0, I, D, G)),
            ("no rows", INVALID, (ctx.h, C.byref(zero), 1, one, T, 0, 0, I, D, G)),
        ]
        for what, code, args in refused:
            assert L.pwn_hip_debug_project_pairs(*args) == code, what
            assert g.value == -9 and (idx == -9).all() and (dep == -9).all(), what
        del foreign
    finally:
        other.close()
    # a cloud of more than 2^21 points (kMaxAlignerPoints), grown on the device: 128 copies of a 2304-point cloud, then copies of those
    I4 = np.eye(4, dtype=F)
    part = cloud_of(ctx, PP.case_named("collide/wide"))
    seed = api.Cloud(ctx, 128 * part.size())
    for _ in range(128):
        seed.add(part, I4)
    big = api.Cloud(ctx, (1 << 21) + seed.size())
    while big.size() <= (1 << 21):
        big.add(seed, I4)
    size = big.size()
    huge = (C.c_void_p * 2)(cloud.h, big.h)
    for which in (0, 1):
        assert L.pwn_hip_debug_project_pairs(ctx.h, P, 2, huge, T, which, 0, I, D, G) == INVALID, "a cloud above 2^21 points"
        assert g.value == -9 and (idx == -9).all() and (dep == -9).all() and big.size() == size
    del big, seed
    # either output may be left out
    assert L.pwn_hip_debug_project_pairs(ctx.h, P, 1, one, T, 0, 0, None, None, G) == 0 and g.value == 0
    assert L.pwn_hip_debug_project_pairs(ctx.h, P, 1, one, T, 0, 0, I, None, G) == 0 and (idx[:N] != -9).all() and (idx[N:] == -9).all() and (dep == -9).all()
