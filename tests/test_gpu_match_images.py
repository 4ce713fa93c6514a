"""k_match_score (the matchClouds score, pwn_tracker/pwn_matcher_base.cpp:153-182) on the injected depth pairs of tests/match_images.py, in every
launch form: the single-pair entry after one alignment, pwn_hip_match_batch with 3 pairs (up to 256 workgroups per pair) and with 9 and 20 (64
per pair, several turns of the grid-stride loop), pwn_hip_match_batch_records into host and device buffers, sub-batches on one and two streams.

Clouds are made both ways: by the converter (they carry their own index image: the batch path reads the current depths off the cloud, curOwn)
and by unProject (no index image: both sides are projected).  With outer_iterations = 1 the finder's images are those of the first projection:
the expected images are oracle.project of the GPU clouds' points -- reference under the guess, current under the identity -- and the expected
score is the integer model's (match_images.score) and the oracle's (oracle.match_score) of those images:

    counts                exact against both
    distance vs model     bit for bit, always (both are the float nearest to the exact sum, divided by the count; NaN for 0/0)
    distance vs oracle    bit for bit while the sum stays at or below 2^18 mm, within (n - 1) 2^-24 relative above (match_images.long_sum_bar)

What each case is there for (a library with the one change fails the tests named): the loop's second turn dropped -- the 264 x 256 single pair
and every batch of 9 or 20 (tail pair); `i <= n - 256` as the loop bound -- everything down to the 24 x 32 table; `out + 0` for the pair's
accumulator -- every batch; the accumulators of a later sub-batch written at the first one's place -- test_sub_batches_and_streams; the two
epoch tags swapped -- test_two_outer_iterations (with one outer iteration the tags are equal); a shift class moved -- every pair with all
classes; 1 mm counted as 1e-37 -- the 1 mm pair; no upward rounding of a tie by 1 mm pixels -- the long sum.  The bounds `ci < ncur` and
`ri < nref` cannot be reached from here: every index a z-buffer or a cloud's own index image holds was written for that cloud's count.
"""
import ctypes as C

import numpy as np
import pytest

import match_images as MI

pytestmark = pytest.mark.gpu

I4 = np.eye(4, dtype=np.float32)


class Rig:
    def __init__(self, oracle):
        from g2o_frontend_amd import api
        self.api, self.O = api, oracle
        self.ctx = api.Context(device=0, max_rows=MI.SINGLE_SHAPE[0], max_cols=MI.SINGLE_SHAPE[1], max_batch=24)
        self._objects, self._clouds, self._points, self._expected = {}, {}, {}, {}

    def close(self):
        self._clouds.clear()
        self.ctx.close()

    def objects(self, shape, image=None, outer=1):
        """(projector, converter, aligner) for frames of `shape`; the aligner's projector describes `image` (default: the frames' size)"""
        key = (shape, image or shape, outer)
        if key not in self._objects:
            api = self.api
            conv, alig = MI.converter_conf(), MI.aligner_conf(outer)

            def projector(size):
                K = MI.camera(*size)
                p = api.PinholePointProjector()
                p.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]); p.setMinDistance(MI.MIN_DISTANCE); p.setMaxDistance(MI.MAX_DISTANCE)
                p.setImageSize(*size)
                return p
            cproj = projector(shape)
            stats = api.StatsCalculatorIntegralImage()
            stats.setWorldRadius(conv["world_radius"]); stats.setMinImageRadius(conv["min_image_radius"]); stats.setMaxImageRadius(conv["max_image_radius"])
            stats.setMinPoints(conv["min_points"]); stats.setCurvatureThreshold(conv["stats_curvature_threshold"])
            pinfo, ninfo = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
            pinfo.setCurvatureThreshold(conv["point_info_curvature_threshold"]); ninfo.setCurvatureThreshold(conv["normal_info_curvature_threshold"])
            converter = api.DepthImageConverterIntegralImage(cproj, stats, pinfo, ninfo)
            aproj = projector(image or shape)
            f = api.CorrespondenceFinder()
            f.setInlierDistanceThreshold(alig["inlier_distance_threshold"]); f.setInlierNormalAngularThreshold(alig["inlier_normal_angular_threshold"])
            f.setFlatCurvatureThreshold(alig["flat_curvature_threshold"]); f.setInlierCurvatureRatioThreshold(alig["inlier_curvature_ratio_threshold"])
            f.setImageSize(*(image or shape))
            lin = api.Linearizer(); lin.setInlierMaxChi2(alig["inlier_max_chi2"]); lin.setRobustKernel(alig["robust_kernel"])
            a = api.Aligner(self.ctx)
            a.setProjector(aproj); a.setLinearizer(lin); a.setCorrespondenceFinder(f)
            a.setOuterIterations(alig["outer_iterations"]); a.setInnerIterations(alig["inner_iterations"])
            self._objects[key] = (cproj, converter, a)
        return self._objects[key]

    def clouds(self, pairs, how):
        """[(reference cloud, current cloud)] of the pairs, made by the converter ("conv") or by unProject ("unproj"); made once per pair"""
        api = self.api
        todo = [p for p in pairs if (p.name, how) not in self._clouds]
        if todo:
            shape = todo[0].ref.shape
            proj, converter, _ = self.objects(shape)
            made = [api.Cloud(self.ctx, shape[0] * shape[1]) for _ in range(2 * len(todo))]
            frames = [p.ref for p in todo] + [p.cur for p in todo]
            if how == "conv":
                for base in range(0, len(made), 24):
                    converter.computeBatch(made[base:base + 24], frames[base:base + 24])
            else:
                for c, fr in zip(made, frames):
                    proj.unProject(c, fr)
            for k, p in enumerate(todo):
                assert made[k].size() == int((p.ref > 0).sum()) and made[len(todo) + k].size() == int((p.cur > 0).sum()), p.name
                self._clouds[(p.name, how)] = (made[k], made[len(todo) + k])
        return [self._clouds[(p.name, how)] for p in pairs]

    def expected(self, pair, how, guess, threshold, image=None):
        """(model score, oracle score) of oracle.project of the pair's GPU clouds: reference under `guess`, current under the identity"""
        key = (pair.name, how, guess.tobytes(), float(threshold), image)
        if key not in self._expected:
            ikey = key[:3] + (image,)
            if ikey not in self._points:
                rc, cc = self._clouds[(pair.name, how)]
                rows, cols = image or pair.ref.shape
                K = MI.camera(rows, cols)
                _, rd = self.O.project(K, guess, MI.MIN_DISTANCE, MI.MAX_DISTANCE, rows, cols, rc.points())
                _, cd = self.O.project(K, I4, MI.MIN_DISTANCE, MI.MAX_DISTANCE, rows, cols, cc.points())
                self._points[ikey] = (rd, cd)
            rd, cd = self._points[ikey]
            self._expected[key] = (MI.score(rd, cd, threshold), self.O.match_score(rd, cd, threshold))
        return self._expected[key]

    # ---- the launch forms
    def _args(self, aligner, cl, guesses):
        n = len(cl)
        refs = (C.c_void_p * n)(*[r.h for r, _ in cl]); curs = (C.c_void_p * n)(*[c.h for _, c in cl])
        g = np.ascontiguousarray(np.stack([self.api._colmajor(np.asarray(T, np.float32), 4) for T in guesses]), np.float32)
        return aligner.params(), n, refs, curs, g

    def batch(self, aligner, cl, guesses, threshold):
        """pwn_hip_match_batch -> ([(nonZeros, inliers, outliers, distance bits)], the raw bytes of the score array, transforms)"""
        p, n, refs, curs, g = self._args(aligner, cl, guesses)
        res, sc = (self.api.AlignResult * n)(), (self.api.MatchResult * n)()
        self.ctx.check(self.ctx._L.pwn_hip_match_batch(self.ctx.h, C.byref(p), n, refs, curs, self.api._ptr(g), threshold, res, sc))
        return [_tuple(s) for s in sc], bytes(sc), [np.array(list(r.T), np.float32).reshape(4, 4).T for r in res]

    def records(self, aligner, cl, guesses, threshold, device):
        """pwn_hip_match_batch_records -> (scores as above, the [n, 72] records as written)"""
        p, n, refs, curs, g = self._args(aligner, cl, guesses)
        res, sc = (self.api.AlignResult * n)(), (self.api.MatchResult * n)()
        host = np.full((n, self.api.MATCH_RECORD_FLOATS), -7.0, np.float32)
        buf = self.ctx.upload(host) if device else host
        self.ctx.check(self.ctx._L.pwn_hip_match_batch_records(self.ctx.h, C.byref(p), n, refs, curs, self.api._ptr(g), threshold, None, 500, res, sc,
                                                               self.api._ptr(buf)))
        out = buf.numpy().copy() if device else host
        if device:
            buf.free()
        return [_tuple(s) for s in sc], out

    def single(self, aligner, ref, cur, guess, thresholds):
        """pwn_hip_align, then pwn_hip_match_score once per threshold"""
        aligner.setReferenceCloud(ref); aligner.setCurrentCloud(cur); aligner.setInitialGuess(guess)
        aligner.align()
        out = []
        for t in thresholds:
            m = self.api.MatchResult()
            self.ctx.check(self.ctx._L.pwn_hip_match_score(self.ctx.h, t, C.byref(m)))
            out.append(_tuple(m))
        return out

    def shortcut(self, on):
        self.ctx.check(self.ctx._L.pwn_hip_debug_set_index_shortcut(self.ctx.h, 1 if on else 0))


def _tuple(m):
    return (m.image_non_zeros, m.image_inliers, m.image_outliers, MI.bits(m.image_reprojection_distance))


def _dist(word):
    return np.array([word], np.uint32).view(np.float32)[0]


def check(tag, got, model, o):
    """one GPU score against the model's and the oracle's of the same images (the rules of the module text)"""
    nz, inl, out, word = got
    d = _dist(word)
    od = np.float32(o["image_reprojectionDistance"])
    print(f"    {tag}: nonZeros {nz} inliers {inl} outliers {out} distance {float(d):.9g} (model {float(model['distance']):.9g}, oracle {float(od):.9g})")
    assert (nz, inl, out) == (model["nonZeros"], model["inliers"], model["outliers"]), (tag, got, model)
    assert (nz, inl, out) == (o["image_nonZeros"], o["image_inliers"], o["image_outliers"]), (tag, got, o)
    assert MI.same_distance(d, model["distance"]), (tag, float(d), float(model["distance"]), hex(word), hex(MI.bits(model["distance"])))
    if nz == 0:
        assert np.isnan(d) and np.isnan(od), tag
    elif model["sum_mm"] <= MI.BITWISE_SUM_MM:
        assert MI.same_distance(d, od), (tag, float(d), float(od))
    else:
        assert abs(float(d) - float(od)) <= MI.long_sum_bar(nz) * float(od), (tag, float(d), float(od))


@pytest.fixture(scope="module")
def rig(oracle):
    r = Rig(oracle)
    yield r
    r.shortcut(True)
    r.close()


def _launches(ctx, stage):
    return ctx.stage_ms(stage)[1]


def _check_batch(rig, pairs, how, aligner, guesses, threshold, image=None, tag=""):
    cl = rig.clouds(pairs, how)
    got, raw, _ = rig.batch(aligner, cl, guesses, threshold)
    for p, g, T in zip(pairs, got, guesses):
        m, o = rig.expected(p, how, np.asarray(T, np.float32), threshold, image)
        check(f"{tag} {how} {p.name} t={threshold}", g, m, o)
    return got, raw


HOW = ("conv", "unproj")


def test_class_table_single_pair_entry(rig):
    """24 x 32, one column per class: the single-pair entry under the closer's threshold, under 2.5 and 3.0 (5 mm -> 2.5, 3 mm -> 3.0) and 0"""
    p = MI.table_pair()
    _, _, aligner = rig.objects(MI.TABLE_SHAPE)
    ths = (50.0, 2.5, 3.0, 0.0)
    for how in HOW:
        (rc, cc), = rig.clouds([p], how)
        got = rig.single(aligner, rc, cc, I4, ths)
        for t, g in zip(ths, got):
            m, o = rig.expected(p, how, I4, t)
            check(f"table {how} t={t}", g, m, o)
            f = MI.score(p.ref, p.cur, t)                              # under the identity the images are the frames
            assert (f["nonZeros"], f["inliers"], f["sum_units"]) == (m["nonZeros"], m["inliers"], m["sum_units"])
        assert got[3][1] == 0 and got[1][1] < got[2][1] < got[0][1] < got[0][0]


def test_single_pair_entry_takes_a_second_turn(rig):
    """264 x 256 = 264 workgroups of pixels under the single-pair entry's cap of 256"""
    p = MI.single_pair()
    _, _, aligner = rig.objects(MI.SINGLE_SHAPE)
    for how in HOW:
        (rc, cc), = rig.clouds([p], how)
        for gk in ("identity", "moved"):
            G = MI.guess(gk)
            got, = rig.single(aligner, rc, cc, G, (50.0,))
            m, o = rig.expected(p, how, G, 50.0)
            check(f"single {how} {gk}", got, m, o)
            assert m["nonZeros"] > 256 * MI.WG - 4000


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("n", [3, 9])
def test_batches_with_the_shortcut_on_and_off(rig, n, how):
    """3 pairs: one launch of 83 workgroups per pair; 9 pairs: 64 per pair, a second, partial turn.  Converter-made clouds with the index
    shortcut on skip the current projection (the score reads the cloud, curOwn); everything else projects.  Same integers either way."""
    pairs = MI.batch_pairs(n)
    _, _, aligner = rig.objects(MI.BATCH_SHAPE)
    ctx = rig.ctx
    ctx.set_subbatch(64, 64); ctx.set_concurrency(1)
    ths = (50.0,) if n == 3 else (50.0, 2.5, 3.0, 0.0)
    seen = {}
    try:
        for on in (True, False):
            rig.shortcut(on)
            ctx.set_profiling(True)
            for t in ths:
                seen[(on, t)] = _check_batch(rig, pairs, how, aligner, [I4] * n, t, tag=f"batch{n} shortcut={int(on)}")
                assert _launches(ctx, "match_score") == 1
                assert _launches(ctx, "project_cur") == (0 if (on and how == "conv") else 1), (on, how)
                assert _launches(ctx, "project_ref") == 1
            ctx.set_profiling(False)
    finally:
        ctx.set_profiling(False); rig.shortcut(True)
    for t in ths:
        assert seen[(True, t)][0] == seen[(False, t)][0]
    if n == 9:
        assert all(g[1] == 0 for g in seen[(True, 0.0)][0])            # strict `<`: a threshold of 0 has no inliers
    # the frames' own score: under the identity the images are the frames
    for p, g in zip(pairs, seen[(True, 50.0)][0]):
        f = MI.score(p.ref, p.cur, 50.0)
        assert (f["nonZeros"], f["inliers"]) == g[:2], p.name
    keys = [g[:2] + (g[3],) for g in seen[(True, 50.0)][0]]
    assert len(set(keys)) == n


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_records_carry_the_scores(rig, device):
    """words 64..67 of the 72-float records: nonZeros, outliers, inliers, distance as the model has them; words 68..71 are 0"""
    pairs = MI.batch_pairs(9)
    _, _, aligner = rig.objects(MI.BATCH_SHAPE)
    rig.ctx.set_subbatch(64, 64); rig.ctx.set_concurrency(1)
    for how in HOW:
        cl = rig.clouds(pairs, how)
        got, rec = rig.records(aligner, cl, [I4] * 9, 50.0, device)
        assert rec.shape == (9, 72)
        for k, (p, g) in enumerate(zip(pairs, got)):
            m, o = rig.expected(p, how, I4, 50.0)
            check(f"records {how} {p.name}", g, m, o)
            w = rec[k, 64:72]
            assert (int(w[0]), int(w[1]), int(w[2])) == (m["nonZeros"], m["outliers"], m["inliers"]), p.name
            assert MI.same_distance(w[3], m["distance"]) and MI.bits(w[3]) == g[3], p.name
            assert not w[4:].view(np.uint32).any(), p.name
            assert rec[k, 19] == 500 + k and not (rec[k] == -7.0).any()


@pytest.mark.parametrize("how", HOW)
def test_sub_batches_and_streams(rig, how):
    """20 pairs as sub-batches of 8 and of 3 (7 sub-batches, workspace slots reused round-robin) on one and on two streams, and as one sub-batch:
    every pair's score is its own, and the reversed list gives the reversed results"""
    pairs = MI.batch_pairs(20)
    _, _, aligner = rig.objects(MI.BATCH_SHAPE)
    ctx = rig.ctx
    first = None
    try:
        for sub, streams in ((8, 1), (8, 2), (3, 1), (3, 2), (20, 1)):
            ctx.set_subbatch(sub, sub); ctx.set_concurrency(streams)
            ctx.set_profiling(True)
            fwd, _ = _check_batch(rig, pairs, how, aligner, [I4] * 20, 50.0, tag=f"sub{sub}x{streams}")
            assert _launches(ctx, "match_score") == (20 + sub - 1) // sub
            ctx.set_profiling(False)
            rev, _ = _check_batch(rig, pairs[::-1], how, aligner, [I4] * 20, 50.0, tag=f"sub{sub}x{streams} reversed")
            assert rev == fwd[::-1]
            first = first or fwd
            assert fwd == first
    finally:
        ctx.set_profiling(False); ctx.set_subbatch(64, 64); ctx.set_concurrency(2)
    assert len({g[:2] + (g[3],) for g in first}) == 20


def test_sub_batches_of_mixed_clouds(rig):
    """a sub-batch reads its current depths off the clouds only if every pair of it can: converter-made and unProject-made clouds in runs of
    three -- sub-batches of 3 alternate between the two forms, sub-batches of 8 all project -- on two streams, the same scores either way"""
    pairs = MI.batch_pairs(20)
    hows = ["conv" if (k // 3) % 2 == 0 else "unproj" for k in range(20)]
    for how in HOW:
        rig.clouds(pairs, how)
    cl = [rig.clouds([p], h)[0] for p, h in zip(pairs, hows)]
    _, _, aligner = rig.objects(MI.BATCH_SHAPE)
    ctx = rig.ctx
    try:
        for sub, projected in ((3, 3), (8, 3)):
            ctx.set_subbatch(sub, sub); ctx.set_concurrency(2); ctx.set_profiling(True)
            got, _, _ = rig.batch(aligner, cl, [I4] * 20, 50.0)
            assert _launches(ctx, "project_cur") == projected and _launches(ctx, "match_score") == (20 + sub - 1) // sub
            for p, h, g in zip(pairs, hows, got):
                m, o = rig.expected(p, h, I4, 50.0)
                check(f"mixed sub{sub} {h} {p.name}", g, m, o)
    finally:
        ctx.set_profiling(False); ctx.set_subbatch(64, 64); ctx.set_concurrency(2)


def _moved(k):
    G = MI.guess("moved").copy()
    G[:2, 3] *= np.float32(1.0 + 0.25 * k)
    return G


@pytest.mark.parametrize("how", HOW)
def test_moved_guesses_and_a_smaller_image(rig, how):
    """a rotation and a translation per pair: the reference depth is row 2 of K R t applied to the point, not its z; and an image half the
    clouds' size, where four points share a pixel and the nearest wins"""
    pairs = MI.batch_pairs(9)
    rig.ctx.set_subbatch(64, 64); rig.ctx.set_concurrency(1)
    guesses = [_moved(k) for k in range(9)]
    _, _, aligner = rig.objects(MI.BATCH_SHAPE)
    got, _ = _check_batch(rig, pairs, how, aligner, guesses, 50.0, tag="moved")
    same, _ = _check_batch(rig, pairs, how, aligner, [I4] * 9, 50.0, tag="identity")
    assert sum(a[:2] != b[:2] for a, b in zip(got, same)) >= 6           # the guess shows in the counts
    half = (MI.BATCH_SHAPE[0] // 2, MI.BATCH_SHAPE[1] // 2)
    _, _, small = rig.objects(MI.BATCH_SHAPE, image=half)
    for gs, tag in ((guesses, "half moved"), ([I4] * 9, "half identity")):
        res, _ = _check_batch(rig, pairs, how, small, gs, 50.0, image=half, tag=tag)
        assert max(r[0] for r in res) <= half[0] * half[1]
    # the single-pair entry under a moved guess, batch shape: 83 workgroups, no second turn, the image ends inside the last one
    for k in (0, 2, 4):
        rc, cc = rig.clouds([pairs[k]], how)[0]
        g, = rig.single(aligner, rc, cc, guesses[k], (50.0,))
        assert g == got[k]


def test_two_outer_iterations(rig):
    """outer_iterations = 2: the score reads the LAST reference projection (its epoch tag is not the current projection's).  unProject-made
    clouds have no normals, so no correspondence, so the pose stays the identity bit for bit: the last projection is the first one's twin and
    the expected score the oracle's.  Converter-made clouds move: there the batch is compared with itself with the shortcut off (the first
    reference projection is then executed instead of taken from the cloud), every integer and bit."""
    pairs = MI.batch_pairs(9)
    rig.ctx.set_subbatch(64, 64); rig.ctx.set_concurrency(1)
    _, _, two = rig.objects(MI.BATCH_SHAPE, outer=2)
    cl = rig.clouds(pairs, "unproj")
    got, _, Ts = rig.batch(two, cl, [I4] * 9, 50.0)
    for p, g, T in zip(pairs, got, Ts):
        assert np.array_equal(T.view(np.uint32), I4.view(np.uint32)), p.name
        m, o = rig.expected(p, "unproj", I4, 50.0)
        check(f"outer2 unproj {p.name}", g, m, o)
    cl = rig.clouds(pairs, "conv")
    try:
        rig.ctx.set_profiling(True)
        on, raw_on, T_on = rig.batch(two, cl, [I4] * 9, 50.0)
        assert _launches(rig.ctx, "project_ref") == 1 and _launches(rig.ctx, "project_cur") == 0      # the first of two skipped
        rig.shortcut(False)
        off, raw_off, T_off = rig.batch(two, cl, [I4] * 9, 50.0)
        assert _launches(rig.ctx, "project_ref") == 2 and _launches(rig.ctx, "project_cur") == 1
    finally:
        rig.ctx.set_profiling(False); rig.shortcut(True)
    assert on == off and raw_on == raw_off
    for a, b in zip(T_on, T_off):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for p, g in zip(pairs, on):
        if p.kind in ("bitwise", "long", "one_mm"):
            assert g[0] > 10000, (p.name, g)                           # the images are there (no comparison with the oracle at a free iterate)


def test_the_same_batch_twice_gives_the_same_bytes(rig):
    """the accumulators are cleared per call"""
    pairs = MI.batch_pairs(9)
    _, _, aligner = rig.objects(MI.BATCH_SHAPE)
    rig.ctx.set_subbatch(4, 4); rig.ctx.set_concurrency(2)
    try:
        for how in HOW:
            cl = rig.clouds(pairs, how)
            a = rig.batch(aligner, cl, [I4] * 9, 50.0)
            b = rig.batch(aligner, cl, [I4] * 9, 50.0)
            assert a[0] == b[0] and a[1] == b[1]
            ra = rig.records(aligner, cl, [I4] * 9, 50.0, False)
            rb = rig.records(aligner, cl, [I4] * 9, 50.0, False)
            assert ra[0] == a[0] and np.array_equal(ra[1][:, 64:].view(np.uint32), rb[1][:, 64:].view(np.uint32))
    finally:
        rig.ctx.set_subbatch(64, 64)
