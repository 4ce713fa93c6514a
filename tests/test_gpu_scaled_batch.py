"""Batches of frames converted and aligned at 1 / step resolution: the batched DepthImage_scale kernel (pwn_hip_depth_scale_batch[_u16]), n x
PwnMatcherBase::makeCloud's data path in one call (pwn_hip_convert_batch[_u16]_scaled), the one-submission step at 1 / step resolution
(pwn_hip_convert_align_batch_u16_scaled) and their Python / C++ mirrors, on the frames of tests/scaled_frames.py.

  * down-sampled images: bit for bit oracle.depth_scale(oracle.convert_16u_to_32f(raw), step), for uint16 and float sources in device memory,
    in pageable host memory and in device memory one element off a 16-byte boundary (the scalar kernel), every frame count of the plan;
  * clouds: pwn_hip_convert_scaled of every frame equals oracle.convert of the oracle-scaled frame in every array and in the stored index image
    (exact9: bit for bit; one configuration in the default sym6, compared as tests/test_omega_sym6.py compares), and the clouds of the batch
    calls equal those of pwn_hip_convert_scaled in every byte of their flat form (points, normals, matrices, index image and its key);
  * several sub-batches on two streams with reused slots, host frames through the copy stream;
  * the step against convert-then-align on other clouds, records in device and in host memory, one pair against the oracle;
  * the mirrors, the refusals and the stage name.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flat_clouds as FC
import scaled_frames as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV = S.MAX_DEPTH_COV
COMBOS = [(kind, where) for kind in ("raw", "float") for where in ("device", "host", "misaligned")]
OK, INVALID, CAPACITY = 0, 1, 6


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Ptr:
    """a frame argument at an address of its own (what _ptr() takes from a tensor)"""
    def __init__(self, address, shape):
        self._a, self.shape = address, shape

    def data_ptr(self): return self._a
    def is_contiguous(self): return True


class Placed:
    """n frames where a call finds them: pageable host memory, device memory at 256-byte boundaries, or device memory one element behind one"""
    def __init__(self, ctx, frames, where):
        self.buf = None
        if where == "host":
            self.keep = [np.array(f, copy=True) for f in frames]      # pageable, one allocation each
            self.args = self.keep
            return
        off = 1 if where == "misaligned" else 0
        item, nb = frames[0].dtype.itemsize, frames[0].nbytes
        pitch = (nb + off * item + 255) // 256 * 256
        block = np.zeros(len(frames) * pitch, np.uint8)
        for i, f in enumerate(frames):
            block[i * pitch + off * item: i * pitch + off * item + nb] = np.ascontiguousarray(f).view(np.uint8).ravel()
        self.buf = ctx.upload(block)
        self.args = [Ptr(self.buf.data_ptr() + i * pitch + off * item, frames[0].shape) for i in range(len(frames))]
        assert all((a.data_ptr() % 16 != 0) == (where == "misaligned") for a in self.args)

    def free(self):
        if self.buf is not None:
            self.buf.free()


def window(n, start):
    return [(start + j) % S.POOL for j in range(n)]


def plan(cfg_index):
    """the six (element type, location) pairs of a configuration, each with one of the five frame counts: every pair and every count occur in
    every configuration, and the pairing moves with the configuration"""
    return [(kind, where, S.COUNTS[(k + cfg_index) % len(S.COUNTS)], 3 * k + cfg_index) for k, (kind, where) in enumerate(COMBOS)]


def make_converter(K):
    """the reference's object graph with oracle.QVGA4_CONF_CONVERTER's values and camera (fx, fy, cx, cy)"""
    from g2o_frontend_amd import api
    from oracle import oracle as O
    conv = O.QVGA4_CONF_CONVERTER
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    proj.setMinDistance(conv["min_distance"]); proj.setMaxDistance(conv["max_distance"])
    stats = api.StatsCalculatorIntegralImage()
    stats.setWorldRadius(conv["world_radius"]); stats.setMinImageRadius(conv["min_image_radius"])
    stats.setMaxImageRadius(conv["max_image_radius"]); stats.setMinPoints(conv["min_points"])
    stats.setCurvatureThreshold(conv["stats_curvature_threshold"])
    pinfo, ninfo = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
    pinfo.setCurvatureThreshold(conv["point_info_curvature_threshold"]); ninfo.setCurvatureThreshold(conv["normal_info_curvature_threshold"])
    return api.DepthImageConverterIntegralImage(proj, stats, pinfo, ninfo)


def make_aligner(ctx, K, rows, cols):
    from g2o_frontend_amd import api
    from oracle import oracle as O
    alig = O.QVGA4_CONF_ALIGNER
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    proj.setMinDistance(O.QVGA4_CONF_CONVERTER["min_distance"]); proj.setMaxDistance(O.QVGA4_CONF_CONVERTER["max_distance"])
    proj.setImageSize(rows, cols)
    finder = api.CorrespondenceFinder()
    finder.setInlierDistanceThreshold(alig["inlier_distance_threshold"]); finder.setInlierNormalAngularThreshold(alig["inlier_normal_angular_threshold"])
    finder.setFlatCurvatureThreshold(alig["flat_curvature_threshold"]); finder.setInlierCurvatureRatioThreshold(alig["inlier_curvature_ratio_threshold"])
    finder.setImageSize(rows, cols)
    lin = api.Linearizer(); lin.setInlierMaxChi2(alig["inlier_max_chi2"]); lin.setRobustKernel(alig["robust_kernel"])
    aligner = api.Aligner(ctx)
    aligner.setProjector(proj); aligner.setLinearizer(lin); aligner.setCorrespondenceFinder(finder)
    aligner.setOuterIterations(alig["outer_iterations"]); aligner.setInnerIterations(alig["inner_iterations"])
    return aligner


flat_bytes, stored_index = FC.flat_bytes, FC.stored_index      # the flat form and its header are read in tests/flat_clouds.py


def scaled_call(ctx, p, kind, args, rows, cols, step, clouds, cov=COV):
    n = len(args)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr() for a in args])
    handles = (C.c_void_p * n)(*[c.h for c in clouds])
    if kind == "raw":
        return ctx._L.pwn_hip_convert_batch_u16_scaled(ctx.h, C.byref(p), ptrs, S.RAW_SCALE, n, rows, cols, step, cov, handles)
    return ctx._L.pwn_hip_convert_batch_scaled(ctx.h, C.byref(p), ptrs, n, rows, cols, step, cov, handles)


def single_scaled(ctx, p, depth, step, cloud):
    rows, cols = depth.shape
    ctx.check(ctx._L.pwn_hip_convert_scaled(ctx.h, C.byref(p), depth.ctypes.data_as(C.c_void_p), rows, cols, step, COV, cloud.h))


def same_cloud_exact9(o, g):
    """tests/test_gpu_parity.py's rule: the oracle's bits in every field (+0 / -0 are the same number)"""
    assert len(o["points"]) == len(g["points"])
    if len(o["points"]) == 0:                  # a signs frame: noise whose blocks the variance test rejects
        return
    for k in ("points", "normals", "curvature", "omega_p", "omega_n"):
        a, b = o[k].reshape(len(o[k]), -1), g[k].reshape(len(g[k]), -1)
        same = (_bits(a) == _bits(b)) | ((a == 0) & (b == 0))
        assert same.all(), f"{k}: {int((~same).any(1).sum())} of {len(a)} points differ"


# ------------------------------------------------------------------------------------------------------------ shared, computed once
@pytest.fixture(scope="module")
def ctx():
    from g2o_frontend_amd import api
    c = api.Context(device=0, max_rows=480, max_cols=640, max_batch=32, omega_storage="exact9")
    c.set_profiling(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pools(oracle):
    """per configuration: the uint16 and float frames and the oracle's down-sampled images, left unchanged"""
    cache = {}

    def get(cfg):
        if cfg not in cache:
            _, step = cfg
            raw = S.raw_pool(cfg)
            flt = S.float_pool(oracle, cfg, raw)
            want_raw = [oracle.depth_scale(oracle.convert_16u_to_32f(f, S.RAW_SCALE), step, COV) for f in raw]
            want_flt = [oracle.depth_scale(f, step, COV) if k in S.SIGNS_AT else want_raw[k] for k, f in enumerate(flt)]
            cache[cfg] = dict(raw=raw, float=flt, want=dict(raw=want_raw, float=want_flt))
        return cache[cfg]
    return get


# ------------------------------------------------------------------------------------------------------------ the down-sampled images
@pytest.mark.parametrize("ci", range(len(S.CONFIGS)), ids=[S.config_id(c) for c in S.CONFIGS])
def test_downsampled_images_bit_exact(ctx, pools, ci):
    cfg = S.CONFIGS[ci]
    (rows, cols), step = cfg
    pool = pools(cfg)
    orows, ocols = rows // step, cols // step
    for k, (kind, where, n, start) in enumerate(plan(ci)):
        frames = window(n, start)
        src = Placed(ctx, [pool[kind][i] for i in frames], where)
        dst_dev = ctx.upload(np.full((n, orows, ocols), -7.0, np.float32)) if k % 2 == 0 else None      # destinations: device and host in turn
        out = [dst_dev.frame(j) for j in range(n)] if dst_dev is not None else [np.full((orows, ocols), -7.0, np.float32) for _ in range(n)]
        ctx.DepthImage_scale_batch(src.args, step, COV, raw_scale=S.RAW_SCALE if kind == "raw" else None, out=out)
        assert ctx.stage_ms("depth_scale")[1] == 1
        got = dst_dev.numpy() if dst_dev is not None else np.stack(out)
        bad = [frames[j] for j in range(n) if not S.same_bits(got[j], pool["want"][kind][frames[j]])]
        assert not bad, (cfg, kind, where, n, bad)
        src.free()
        if dst_dev is not None:
            dst_dev.free()


def test_more_frames_than_slots_go_in_chunks(pools):
    """a context of 4 slots takes 9 host frames in three launches; its results are those of the large context"""
    from g2o_frontend_amd import api
    cfg = ((121, 163), 3)
    pool = pools(cfg)
    small = api.Context(0, 121, 163, 4, omega_storage="exact9")
    small.set_profiling(True)
    frames = window(9, 2)
    got = small.DepthImage_scale_batch([pool["raw"][i] for i in frames], 3, COV, raw_scale=S.RAW_SCALE)
    assert small.stage_ms("depth_scale")[1] == 3
    assert all(S.same_bits(g, pool["want"]["raw"][i]) for g, i in zip(got, frames))
    small.close()


# ------------------------------------------------------------------------------------------------------------ the clouds
@pytest.fixture(scope="module")
def references(ctx, oracle, pools):
    """per configuration and frame: pwn_hip_convert_scaled's cloud, compared with the oracle's cloud of the oracle-scaled frame (every array and
    the stored index image); kept: that cloud's flat form, which the batch calls' clouds must equal byte for byte.  The oracle converts a
    240 x 320 frame in a third of a second, so at 480 x 640 it is asked for a room frame, a ladder frame and a signs frame and at the small
    shapes for every frame; the down-sampled images of all frames are compared with the oracle's at every shape (above)."""
    from g2o_frontend_amd import api, synth
    cache = {}

    def get(cfg):
        if cfg in cache:
            return cache[cfg]
        (rows, cols), step = cfg
        pool = pools(cfg)
        Ks = synth.scaled_K(S.camera(rows, cols), step)
        cp = oracle.converter_params(K=Ks, **oracle.QVGA4_CONF_CONVERTER)
        p = make_converter(Ks).params(None)
        orows, ocols = rows // step, cols // step
        flats = dict(raw=[], float=[])
        normals = 0
        asked = range(S.POOL) if rows * cols < 100000 else (0, S.ROOM_FRAMES, S.SIGNS_AT[0])
        cloud = api.Cloud(ctx, orows * ocols)
        for k in range(S.POOL):
            depth = oracle.convert_16u_to_32f(pool["raw"][k], S.RAW_SCALE)
            single_scaled(ctx, p, depth, step, cloud)
            r, c, K, idx = stored_index(cloud)
            assert (r, c) == (orows, ocols) and np.array_equal(K, p.K)
            if k in asked and k != S.SIGNS_AT[0]:
                oc, oidx, _ = oracle.convert(cp, pool["want"]["raw"][k])
                o = oc.arrays()
                same_cloud_exact9(o, cloud.arrays())
                assert np.array_equal(idx, oidx)
                normals += int((np.abs(o["normals"][:, :3]).sum(1) > 0).sum())
            flats["raw"].append(flat_bytes(cloud))
            if k in S.SIGNS_AT:
                single_scaled(ctx, p, pool["float"][k], step, cloud)
                if k in asked:
                    oc, oidx, _ = oracle.convert(cp, pool["want"]["float"][k])
                    same_cloud_exact9(oc.arrays(), cloud.arrays())
                    assert np.array_equal(stored_index(cloud)[3], oidx)
                flats["float"].append(flat_bytes(cloud))
            else:
                flats["float"].append(flats["raw"][k])
        assert normals >= 100, "degenerate input: no normals to compare"
        cache[cfg] = (p, flats)
        return cache[cfg]
    return get


@pytest.mark.parametrize("ci", range(len(S.CONFIGS)), ids=[S.config_id(c) for c in S.CONFIGS])
def test_batch_clouds_equal_single_conversions_and_oracle(ctx, pools, references, ci):
    from g2o_frontend_amd import api
    cfg = S.CONFIGS[ci]
    (rows, cols), step = cfg
    pool = pools(cfg)
    p, flats = references(cfg)
    N = (rows // step) * (cols // step)
    clouds = [api.Cloud(ctx, N) for _ in range(S.POOL)]
    for kind, where, n, start in plan(ci):
        frames = window(n, start + 1)
        src = Placed(ctx, [pool[kind][i] for i in frames], where)
        assert scaled_call(ctx, p, kind, src.args, rows, cols, step, clouds[:n]) == OK, ctx._L.pwn_hip_last_error_string(ctx.h)
        assert ctx.stage_ms("depth_scale")[1] == 1 and ctx.stage_ms("stats")[1] == 1
        bad = [frames[j] for j in range(n) if not np.array_equal(flat_bytes(clouds[j]), flats[kind][frames[j]])]
        assert not bad, (cfg, kind, where, n, bad)
        src.free()


def test_one_configuration_in_the_default_sym6(oracle, pools):
    """121 x 163 at step 2 with sym6 clouds: the batch call's clouds against the oracle's as tests/test_omega_sym6.py compares"""
    from g2o_frontend_amd import api, synth
    from test_omega_sym6 import compare_clouds_sym6
    cfg = ((121, 163), 2)
    (rows, cols), step = cfg
    pool = pools(cfg)
    c6 = api.Context(0, rows, cols, 16)
    assert c6.omega_storage == "sym6"
    Ks = synth.scaled_K(S.camera(rows, cols), step)
    cp = oracle.converter_params(K=Ks, **oracle.QVGA4_CONF_CONVERTER)
    p = make_converter(Ks).params(None)
    frames = window(9, 0)
    clouds = [api.Cloud(c6, (rows // step) * (cols // step)) for _ in frames]
    src = Placed(c6, [pool["raw"][i] for i in frames], "device")
    assert scaled_call(c6, p, "raw", src.args, rows, cols, step, clouds) == OK
    for j, i in enumerate(frames):
        oc, oidx, _ = oracle.convert(cp, pool["want"]["raw"][i])
        compare_clouds_sym6(oc.arrays(), clouds[j].arrays())
        assert np.array_equal(stored_index(clouds[j])[3], oidx)
    src.free()
    c6.close()


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("kind", ["raw", "float"])
def test_several_sub_batches_on_two_streams_reuse_their_slots(oracle, kind, where):
    """13 room frames from 13 seeds, sub-batches of 4 frames on 2 streams in a context of 8 slots: every slot is used twice, by both streams in
    turn; host frames travel on the copy stream.  A stale slot would hold another seed's frame."""
    from g2o_frontend_amd import api, synth
    (rows, cols), step = (121, 163), 2
    ctx = api.Context(0, rows, cols, 8, omega_storage="exact9")
    ctx.set_profiling(True)
    Ks = synth.scaled_K(S.camera(rows, cols), step)
    p = make_converter(Ks).params(None)
    raw = [S.room(rows, cols, 100 + s) for s in range(13)]
    depth = [oracle.convert_16u_to_32f(f, S.RAW_SCALE) for f in raw]
    N = (rows // step) * (cols // step)
    want = []
    one = api.Cloud(ctx, N)
    for d in depth:
        single_scaled(ctx, p, d, step, one)
        want.append(flat_bytes(one))
    assert len({w.tobytes() for w in want}) == 13
    ctx.set_subbatch(4, 4); ctx.set_concurrency(2)
    clouds = [api.Cloud(ctx, N) for _ in range(13)]
    src = Placed(ctx, raw if kind == "raw" else depth, where)
    for _ in range(2):                       # the second call finds every slot filled by the first
        assert scaled_call(ctx, p, kind, src.args, rows, cols, step, clouds) == OK, ctx._L.pwn_hip_last_error_string(ctx.h)
        assert ctx.stage_ms("depth_scale")[1] == 4
        bad = [j for j in range(13) if not np.array_equal(flat_bytes(clouds[j]), want[j])]
        assert not bad, bad
        src.args.reverse(); want.reverse()   # ... with the frames in the opposite order
    src.free()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ the step
RESULT_FIELDS = ("T", "chi2", "iter_inliers", "iter_correspondences", "iter_candidates", "error", "inliers", "iterations", "n_reference", "n_current")


def same_results(got, want):
    for k in RESULT_FIELDS:
        a, b = got[k], want[k]
        assert np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b), k


@pytest.mark.parametrize("step,n", [(4, 6), (2, 5)])
def test_scaled_step_equals_scaled_convert_then_align(oracle, step, n):
    """VGA pairs, sub-batches of 2 pairs: results and records of the one-submission step against pwn_hip_convert_batch_u16_scaled followed by
    pwn_hip_align_batch_records on other clouds, the records in a device and in a host buffer; one pair against the oracle on the oracle's
    scaled clouds (first iteration: K, C and inliers)"""
    from g2o_frontend_amd import api, shard, synth
    rows, cols = 480, 640
    orows, ocols = rows // step, cols // step
    Ks = synth.scaled_K(synth.K_VGA, step)
    ctx = api.Context(0, rows, cols, 16, omega_storage="exact9")
    converter = make_converter(Ks)
    aligner = make_aligner(ctx, Ks, orows, ocols)
    pairs = [synth.make_pair(7100 + s, rows, cols, synth.K_VGA) for s in range(n)]
    rf = [ctx.upload(pr[0]) for pr in pairs]; cf = [ctx.upload(pr[1]) for pr in pairs]
    N = orows * ocols
    mk = lambda: [api.Cloud(ctx, N) for _ in range(n)]      # noqa: E731
    ids = np.arange(300, 300 + n, dtype=np.int32)
    # two calls with a host wait between them
    refs, curs = mk(), mk()
    p = converter.params(None)
    ctx.set_subbatch(4, 2); ctx.set_concurrency(2)
    assert scaled_call(ctx, p, "raw", rf + cf, rows, cols, step, refs + curs) == OK
    want_rec = np.full((n, shard.RECORD_FLOATS), -7.0, np.float32)
    want = aligner.alignBatchRecords(refs, curs, want_rec, pair_ids=ids).copy()
    assert (want["inliers"] > 1000).all(), "degenerate input: the pairs did not align"
    # one submission, other clouds; records on the host, then in device memory, then through prepared handles
    refs2, curs2 = mk(), mk()
    rec = np.full((n, shard.RECORD_FLOATS), -7.0, np.float32)
    got = aligner.convertAlignBatch(converter, refs2, curs2, rf, cf, raw_scale=S.RAW_SCALE, records=rec, pair_ids=ids, step=step, max_depth_cov=COV)
    same_results(got, want)
    assert np.array_equal(_bits(rec), _bits(want_rec))
    dev = ctx.upload(np.full((n, shard.RECORD_FLOATS), -3.0, np.float32))
    prepared = aligner.convertAlignHandles(refs2, curs2, rf, cf, converter=converter, step=step, max_depth_cov=COV)
    got = aligner.convertAlignBatch(converter, None, None, None, None, raw_scale=S.RAW_SCALE, records=dev, pair_ids=ids, prepared=prepared)
    same_results(got, want)
    assert np.array_equal(_bits(dev.numpy()), _bits(want_rec))
    for a, b in zip(refs + curs, refs2 + curs2):
        assert np.array_equal(flat_bytes(a), flat_bytes(b))
    # host frames give the same
    got = aligner.convertAlignBatch(converter, refs2, curs2, [pr[0] for pr in pairs], [pr[1] for pr in pairs], raw_scale=S.RAW_SCALE, step=step)
    same_results(got, want)
    # pair 1 against the oracle
    cp = oracle.converter_params(K=Ks, **oracle.QVGA4_CONF_CONVERTER)
    ap = oracle.aligner_params(orows, ocols, K=Ks, accumulate_fp64=1, **oracle.QVGA4_CONF_ALIGNER)
    scaled = [oracle.depth_scale(oracle.convert_16u_to_32f(f, S.RAW_SCALE), step, COV) for f in pairs[1][:2]]
    oref, _, _ = oracle.convert(cp, scaled[0]); ocur, _, _ = oracle.convert(cp, scaled[1])
    same_cloud_exact9(oref.arrays(), refs2[1].arrays()); same_cloud_exact9(ocur.arrays(), curs2[1].arrays())
    o = oracle.align(ap, oref, ocur)
    it0 = o["iterations"][0]
    assert (got["iter_candidates"][1][0], got["iter_correspondences"][1][0], got["iter_inliers"][1][0]) == (it0["K"], it0["C"], it0["inliers"])
    for f in rf + cf + [dev]:
        f.free()
    ctx.close()


def test_step_one_gives_the_bits_of_the_unscaled_step():
    from g2o_frontend_amd import api, synth
    from conftest import case_params
    from test_gpu_parity import gpu_objects
    rows, cols, K, _, _ = case_params("small")
    n = 5
    ctx = api.Context(0, rows, cols, 8, omega_storage="exact9")
    ctx.set_profiling(True)
    _, converter, aligner = gpu_objects(ctx, "small")
    pairs = [synth.make_pair(7000 + s, rows, cols, K) for s in range(n)]
    rf = [pr[0] for pr in pairs]; cf = [pr[1] for pr in pairs]
    mk = lambda: [api.Cloud(ctx, rows * cols) for _ in range(n)]      # noqa: E731
    refs, curs, refs2, curs2 = mk(), mk(), mk(), mk()
    ctx.set_subbatch(4, 2); ctx.set_concurrency(2)
    want = aligner.convertAlignBatch(converter, refs, curs, rf, cf, raw_scale=S.RAW_SCALE).copy()
    assert ctx.stage_ms("depth_scale")[1] == 0
    cp, p = converter.params(None), aligner.params()
    res = (api.AlignResult * n)()
    arr = lambda xs: (C.c_void_p * n)(*xs)      # noqa: E731
    rc = ctx._L.pwn_hip_convert_align_batch_u16_scaled(ctx.h, C.byref(cp), C.byref(p), n, arr([f.ctypes.data for f in rf]), arr([f.ctypes.data for f in cf]),
                                                      S.RAW_SCALE, rows, cols, arr([c.h for c in refs2]), arr([c.h for c in curs2]), None, None, 0, res, None, 1, COV)
    assert rc == OK, ctx._L.pwn_hip_last_error_string(ctx.h)
    assert ctx.stage_ms("depth_scale")[1] > 0
    same_results(np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=n), want)
    for a, b in zip(refs + curs, refs2 + curs2):
        assert np.array_equal(flat_bytes(a), flat_bytes(b))
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ the mirrors
def _matcher(ctx, scale):
    from g2o_frontend_amd import api, synth
    converter = make_converter(synth.K_VGA)
    aligner = make_aligner(ctx, synth.K_VGA, 0, 0)
    m = api.PwnMatcherBase(aligner, converter)
    m.setScale(scale)
    return m


def test_make_cloud_batch_equals_make_cloud(pools):
    from g2o_frontend_amd import api
    cfg = ((121, 163), 2)
    (rows, cols), step = cfg
    pool = pools(cfg)
    ctx = api.Context(0, rows, cols, 16, omega_storage="exact9")
    m = _matcher(ctx, step)
    fx, fy, cx, cy = S.camera(rows, cols)
    Kmat = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
    off = np.eye(4, dtype=np.float32)
    frames = window(9, 3)
    single = [m.makeCloud(Kmat, off, pool["float"][i]) for i in frames]
    assert m.numCalls == 9
    clouds, r, c, Ks = m.makeCloudBatch(Kmat, off, [pool["float"][i] for i in frames])
    assert m.numCalls == 18 and (r, c) == single[-1][1:3] and np.array_equal(Ks, single[-1][3])
    proj = m.converter().projector()
    assert (proj.imageRows(), proj.imageCols()) == (rows // step, cols // step) and np.array_equal(proj.transform(), np.eye(4, dtype=np.float32))
    for (s, _, _, _), b in zip(single, clouds):
        assert np.array_equal(flat_bytes(s), flat_bytes(b))
    assert sum(s.size() for s, _, _, _ in single) > 1000, "degenerate input: hardly a point to compare"
    raw_clouds = m.makeCloudBatch(Kmat, off, [pool["raw"][i] for i in frames], raw_scale=S.RAW_SCALE, clouds=clouds)[0]
    assert raw_clouds == clouds and m.numCalls == 27
    for j, i in enumerate(frames):
        if i not in S.SIGNS_AT:
            assert np.array_equal(flat_bytes(single[j][0]), flat_bytes(clouds[j]))
    assert m.makeCloudBatch(Kmat, off, [])[0] == []
    ctx.close()


def test_cloud_cache_get_batch_equals_per_key_gets(pools):
    """two caches over the same frames: keys fetched one by one and as batches -- the same clouds, LRU order and hit / miss counts, with a
    repeated key, a resident key that an earlier miss of the batch evicts, and frames of two shapes in one batch"""
    from g2o_frontend_amd import api
    big, small = ((121, 163), 2), ((65, 131), 2)
    ctx = api.Context(0, 121, 163, 16, omega_storage="exact9")
    off = np.eye(4, dtype=np.float32)

    def kmat(rows, cols):
        fx, fy, cx, cy = S.camera(rows, cols)
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
    caches = []
    for _ in range(2):
        m = _matcher(ctx, 2)
        cache = api.CloudCache(m, capacity=4)
        for k in range(6):
            cache.addFrame(("big", k), pools(big)["float"][k], kmat(121, 163), off)
        for k in range(3):
            cache.addFrame(("small", k), pools(small)["float"][k], kmat(65, 131), off)
        caches.append((cache, m))
    (one, m1), (bat, m2) = caches
    batches = [[("big", 0), ("big", 1), ("small", 0)],
               [("big", 1), ("big", 2), ("big", 2), ("small", 1), ("big", 3), ("big", 0), ("big", 1)],
               [("big", 1), ("big", 0)], []]
    for keys in batches:
        want = [one.get(k) for k in keys]
        got = bat.getBatch(keys)
        assert len(got) == len(want)
        for a, b in zip(want, got):
            assert np.array_equal(flat_bytes(a), flat_bytes(b))
        assert list(one._clouds) == list(bat._clouds) and (one.hits, one.misses) == (bat.hits, bat.misses)
    assert (one.hits, one.misses) == (4, 8) and m2.numCalls <= m1.numCalls
    ctx.close()


def test_cpp_check_tool_builds_and_finds_no_difference():
    from g2o_frontend_amd import build
    build.build_tools()
    exe = os.path.join(ROOT, "tools", "pwn_hip_scaled_batch_check")
    for args in (["121", "163", "2", "9"], ["120", "160", "4", "17"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert " 0 differences" in r.stdout


# ------------------------------------------------------------------------------------------------------------ refusals, stage name
def test_refusals_leave_the_clouds_untouched(oracle, pools):
    from g2o_frontend_amd import api, synth
    cfg = ((121, 163), 2)
    (rows, cols), step = cfg
    pool = pools(cfg)
    ctx = api.Context(0, rows, cols, 8, omega_storage="exact9")
    Ks = synth.scaled_K(S.camera(rows, cols), step)
    converter = make_converter(Ks)
    p = converter.params(None)
    orows, ocols = rows // step, cols // step
    N = orows * ocols
    n = 3
    clouds = [api.Cloud(ctx, N) for _ in range(n)]
    raw = [pool["raw"][i] for i in range(n)]; flt = [pool["float"][i] for i in range(n)]
    assert scaled_call(ctx, p, "raw", raw, rows, cols, step, clouds) == OK
    before = [flat_bytes(c) for c in clouds]
    sizes = [c.size() for c in clouds]
    other = [pool["raw"][10 + i] for i in range(n)]      # what a call that went through would convert

    def untouched():
        assert [c.size() for c in clouds] == sizes
        assert all(np.array_equal(flat_bytes(c), b) for c, b in zip(clouds, before))

    class Null:
        h = None
    ctx.set_omega_storage("sym6"); mixed = api.Cloud(ctx, N); ctx.set_omega_storage("exact9")
    ptrs = lambda fr: (C.c_void_p * n)(*[f.ctypes.data if f is not None else None for f in fr])      # noqa: E731
    hs = lambda cl: (C.c_void_p * n)(*[c.h for c in cl])      # noqa: E731
    L = ctx._L
    cases = [
        ("step 0", lambda: scaled_call(ctx, p, "raw", other, rows, cols, 0, clouds), INVALID),
        ("step -2", lambda: scaled_call(ctx, p, "float", flt, rows, cols, -2, clouds), INVALID),
        ("scaled image of zero rows", lambda: scaled_call(ctx, p, "raw", other, rows, cols, rows + 1, clouds), INVALID),
        ("null frame", lambda: L.pwn_hip_convert_batch_u16_scaled(ctx.h, C.byref(p), ptrs([other[0], None, other[2]]), S.RAW_SCALE, n, rows, cols, step, COV, hs(clouds)), INVALID),
        ("null cloud", lambda: L.pwn_hip_convert_batch_u16_scaled(ctx.h, C.byref(p), ptrs(other), S.RAW_SCALE, n, rows, cols, step, COV, hs([clouds[0], Null, clouds[2]])), INVALID),
        ("mixed omega storages", lambda: scaled_call(ctx, p, "raw", other, rows, cols, step, [clouds[0], clouds[1], mixed]), INVALID),
        ("context smaller than the source", lambda: scaled_call(ctx, p, "raw", other, 2 * rows, cols, step, clouds), CAPACITY),
        ("context narrower than the source", lambda: scaled_call(ctx, p, "float", flt, rows // 4, cols * 4, step, clouds), CAPACITY),
    ]
    for name, call, status in cases:
        assert call() == status, name
        assert L.pwn_hip_last_error_string(ctx.h)
        untouched()
    # the image calls
    dst = [np.zeros((orows, ocols), np.float32) for _ in range(n)]
    dp = (C.c_void_p * n)(*[d.ctypes.data for d in dst])
    assert L.pwn_hip_depth_scale_batch_u16(ctx.h, ptrs(raw), S.RAW_SCALE, n, rows, cols, 0, COV, dp) == INVALID
    assert L.pwn_hip_depth_scale_batch(ctx.h, ptrs(flt), n, rows, cols, rows + 1, COV, dp) == INVALID
    assert L.pwn_hip_depth_scale_batch(ctx.h, ptrs([flt[0], None, flt[2]]), n, rows, cols, step, COV, dp) == INVALID
    assert L.pwn_hip_depth_scale_batch(ctx.h, ptrs(flt), n, 2 * rows, cols, step, COV, dp) == CAPACITY
    assert all((d == 0).all() for d in dst)
    # the step: a mismatching aligner size, and the cases above through it
    aligner = make_aligner(ctx, Ks, orows, ocols)
    refs, curs = clouds[:1], clouds[1:2]
    res = (api.AlignResult * 1)()
    one = lambda xs: (C.c_void_p * 1)(*xs)      # noqa: E731

    def step_call(ap, st, r=rows, c=cols, ref_frame=other[0], cur_cloud=curs[0]):
        return L.pwn_hip_convert_align_batch_u16_scaled(ctx.h, C.byref(p), C.byref(ap), 1, one([ref_frame.ctypes.data if ref_frame is not None else None]),
                                                        one([other[1].ctypes.data]), S.RAW_SCALE, r, c, one([refs[0].h]), one([cur_cloud.h]), None, None, 0, res,
                                                        None, st, COV)
    good = aligner.params()
    aligner.correspondenceFinder().setImageSize(rows, cols); aligner.projector().setImageSize(rows, cols)
    full = aligner.params()
    for name, call, status in [("aligner at the source size", lambda: step_call(full, step), INVALID),
                               ("step 0", lambda: step_call(good, 0), INVALID),
                               ("null frame", lambda: step_call(good, step, ref_frame=None), INVALID),
                               ("mixed omega storages", lambda: step_call(good, step, cur_cloud=mixed), INVALID),
                               ("context smaller than the source", lambda: step_call(good, step, r=2 * rows), CAPACITY)]:
        assert call() == status, name
        untouched()
    # a cloud smaller than its number of valid scaled pixels: the frames are counted before anything is written
    corner = np.zeros((rows, cols), np.uint16); corner[:12, :12] = other[0][:12, :12]
    tiny = api.Cloud(ctx, 50)
    assert scaled_call(ctx, p, "raw", [corner], rows, cols, step, [tiny]) == OK and 20 <= tiny.size() <= 36
    held = flat_bytes(tiny)
    for kind, frames, cl in (("raw", other[:2], [clouds[0], tiny]), ("float", flt[:2], [tiny, clouds[1]])):
        assert scaled_call(ctx, p, kind, frames, rows, cols, step, cl) == CAPACITY, kind
        assert np.array_equal(flat_bytes(tiny), held)
        untouched()
    assert step_call(good, step, cur_cloud=tiny) == CAPACITY
    assert np.array_equal(flat_bytes(tiny), held)
    untouched()
    # and the context still converts
    assert scaled_call(ctx, p, "raw", raw, rows, cols, step, clouds) == OK
    untouched()
    ctx.close()


def test_stage_name_and_launch_counts(pools):
    """pwn_hip_last_stage_ms reports the box kernel as `depth_scale`, once per launch: per sub-batch of a scaled call, never for an unscaled one"""
    from g2o_frontend_amd import api, synth
    cfg = ((121, 163), 2)
    (rows, cols), step = cfg
    pool = pools(cfg)
    ctx = api.Context(0, rows, cols, 16, omega_storage="exact9")
    ctx.set_profiling(True)
    converter = make_converter(synth.scaled_K(S.camera(rows, cols), step))
    p = converter.params(None)
    clouds = [api.Cloud(ctx, rows * cols) for _ in range(9)]
    raw = [pool["raw"][i] for i in range(9)]
    ctx.set_subbatch(4, 4); ctx.set_concurrency(1)
    assert scaled_call(ctx, p, "raw", raw, rows, cols, step, clouds) == OK
    ms, launches = ctx.stage_ms("depth_scale")
    assert launches == 3 and ms > 0.0 and ctx.stage_ms("stats")[1] == 3
    ctx.set_subbatch(64, 64)
    assert scaled_call(ctx, p, "raw", raw, rows, cols, step, clouds) == OK
    assert ctx.stage_ms("depth_scale")[1] == 1
    converter.computeBatch(clouds, raw, raw_scale=S.RAW_SCALE)
    assert ctx.stage_ms("depth_scale") == (0.0, 0) and ctx.stage_ms("stats")[1] == 1
    ctx.close()
