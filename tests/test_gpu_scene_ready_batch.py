"""Scene-ready clouds from the batch converter (pwn_hip_convert_batch_ex): Stats and sensor-noise Gaussians inside the batch submission.

  * against the per-frame route, in every bit: pwn_hip_convert(keep_stats = 1) + pwn_hip_cloud_gaussians on the float image the front end read
    (pwn_hip_depth_u16_to_f32, pwn_hip_depth_scale_batch[_u16]) -- every downloaded array, Stats, the five Gaussian arrays, the counts and the
    flat form (which carries the stored index image), for float and uint16 frames in device and pageable host memory, with and without a sensor
    offset, exact9 and sym6, frame counts on both sides of the single-pass threshold, unscaled and scaled shapes;
  * against the oracle (exact9): oracle.convert with set_gaussians(True), Stats and Gaussians bit for bit;
  * no extras = the existing call: flat bytes, no Stats, no Gaussians, the same stage names;
  * slot reuse and sub-batches on two streams; the two store forms of the kernel; content transitions; refusals;
  * the Python mirror's options; CloudCache(sceneReady=True) -> PwnMerger.mergeNodeList -> Merger.merge, and the C++ mirror's check tool.
"""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_frames as DF      # noqa: E402
import scaled_frames as S      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
OK, INVALID, CAPACITY = 0, 1, 6
BASELINE, ALPHA = 0.075, 0.1
COV = S.MAX_DEPTH_COV
UNSCALED = [(9, 65), (17, 129), (65, 130), (129, 513)]
SCALED = [((34, 136), 2), ((121, 163), 3), ((18, 40), 1), ((480, 640), 2)]
COUNTS = (1, 7, 15, 16, 17, 25)      # the latency front end up to 15, the single pass from 16 (kSinglePassMinFrames), partial groups
POOL = max(COUNTS)
CLOUD_KEYS = ("points", "normals", "curvature", "omega_p", "omega_n", "stats", "eigenvalues", "npoints")
GAUSS_KEYS = ("mean", "cov", "info_vec", "info", "flags")
STAGES = ("depth_scale", "unproject", "integral", "integral_rows", "integral_cols", "stats", "gaussians")


def sensor_offset():
    """0.1 m and 10 degrees: enough for gauss_transform to run"""
    a = np.deg2rad(10.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T[:3, 3] = [0.1, 0.0, 0.0]
    return T.astype(F)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def vp(a):
    return None if a is None else (a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else C.c_void_p(a.data_ptr()))


def extras(keep_stats=1, gaussians=1, baseline=BASELINE, alpha=ALPHA):
    from g2o_frontend_amd import _lib
    return _lib.ConvertExtras(keep_stats, gaussians, baseline, alpha)


def batch_ex(ctx, p, frames, raw_scale, rows, cols, step, clouds, ex, frame_ptrs=None, handles=None):
    """pwn_hip_convert_batch_ex -> status.  frames: numpy arrays (host) or objects with data_ptr() (device); raw_scale None = float frames"""
    n = len(clouds)
    ptrs = frame_ptrs if frame_ptrs is not None else (C.c_void_p * max(1, n))(*[f.ctypes.data if isinstance(f, np.ndarray) else f.data_ptr() for f in frames])
    h = handles if handles is not None else (C.c_void_p * max(1, n))(*[c.h for c in clouds])
    return ctx._L.pwn_hip_convert_batch_ex(ctx.h, C.addressof(p), ptrs, 0 if raw_scale is None else 1, raw_scale or 0.0, n, rows, cols, step, COV,
                                           None if ex is None else C.byref(ex), h)


def existing_call(ctx, p, frames, raw_scale, rows, cols, step, clouds):
    n = len(clouds)
    ptrs = (C.c_void_p * n)(*[f.ctypes.data if isinstance(f, np.ndarray) else f.data_ptr() for f in frames])
    h = (C.c_void_p * n)(*[c.h for c in clouds])
    L, a = ctx._L, C.addressof(p)
    if step == 0:
        return L.pwn_hip_convert_batch(ctx.h, a, ptrs, n, rows, cols, h) if raw_scale is None else L.pwn_hip_convert_batch_u16(ctx.h, a, ptrs, raw_scale, n, rows, cols, h)
    if raw_scale is None:
        return L.pwn_hip_convert_batch_scaled(ctx.h, a, ptrs, n, rows, cols, step, COV, h)
    return L.pwn_hip_convert_batch_u16_scaled(ctx.h, a, ptrs, raw_scale, n, rows, cols, step, COV, h)


def flat_bytes(cloud):
    buf = np.zeros(cloud.flatSize(), np.uint8)
    assert cloud.exportFlat(buf) == buf.size
    return buf.tobytes()


def has_stats(cloud):
    from g2o_frontend_amd import _lib
    try:
        cloud.arrays(stats=True)
        return True
    except _lib.PwnHipError:
        return False


def state(cloud):
    """what a refused call must leave alone: flat bytes, size, Stats state, Gaussian count"""
    return flat_bytes(cloud), cloud.size(), has_stats(cloud), cloud.numGaussians()


def snapshot(cloud, stats=True):
    """every downloaded byte of a cloud: arrays (with Stats), Gaussians, counts, flat form"""
    out = {k: v.tobytes() for k, v in cloud.arrays(stats=stats).items()}
    g = cloud.gaussians()
    out.update({"gauss_" + k: g[k].tobytes() for k in GAUSS_KEYS})
    out["size"], out["num_gaussians"], out["flat"] = cloud.size(), cloud.numGaussians(), flat_bytes(cloud)
    return out


def differing(a, b):
    return [k for k in a if a[k] != b[k]]


def float_images(ctx, frames, raw_scale, step):
    """the image the front end reads, made on the device by the library's own calls -> host float arrays"""
    n = len(frames)
    if step:
        rows, cols = frames[0].shape
        out = [np.full((rows // step, cols // step), -7.0, F) for _ in range(n)]
        for base in range(0, n, 8):
            ctx.DepthImage_scale_batch(list(frames[base:base + 8]), step, COV, raw_scale=raw_scale, out=out[base:base + 8])
        return out
    if raw_scale is None:
        return [np.ascontiguousarray(f, F) for f in frames]
    out = []
    for f in frames:
        o = np.full(f.shape, -7.0, F)
        ctx.check(ctx._L.pwn_hip_depth_u16_to_f32(ctx.h, vp(np.ascontiguousarray(f)), vp(o), f.size, raw_scale))
        out.append(o)
    return out


def per_frame(ctx, p, image):
    """the route that existed: pwn_hip_convert(keep_stats = 1), then pwn_hip_cloud_gaussians on the same float image"""
    from g2o_frontend_amd import api
    rows, cols = image.shape
    c = api.Cloud(ctx, rows * cols)
    ctx.check(ctx._L.pwn_hip_convert(ctx.h, C.addressof(p), vp(image), rows, cols, c.h, None, None, 1))
    ctx.check(ctx._L.pwn_hip_cloud_gaussians(ctx.h, C.addressof(p), vp(image), rows, cols, c.h, BASELINE, ALPHA))
    return c


def same_as_oracle(o, g, what):
    """tests/test_scene.py's rule: every array with Stats and the Gaussians bit for bit (+0 / -0 are the same number in the arrays)"""
    oa, ga = o.arrays(stats=True), g.arrays(stats=True)
    assert len(o) == g.size(), what
    if len(o) == 0:                  # an all-invalid frame
        assert g.numGaussians() == 0 == o.num_gaussians(), what
        return
    for k in oa:
        a, b = oa[k].reshape(len(oa[k]), -1), ga[k].reshape(len(ga[k]), -1)
        same = (_bits(a) == _bits(b)) | ((a == 0) & (b == 0))
        assert same.all(), (what, k, int((~same).any(1).sum()))
    og, gg = o.gaussians(), g.gaussians()
    assert o.num_gaussians() == g.numGaussians(), what
    assert np.array_equal(og["flags"], gg["flags"]), what
    m, i = (og["flags"] & 1) != 0, (og["flags"] & 2) != 0
    assert np.array_equal(_bits(og["mean"][m]), _bits(gg["mean"][m])) and np.array_equal(_bits(og["cov"][m]), _bits(gg["cov"][m])), what
    assert np.array_equal(_bits(og["info"][i]), _bits(gg["info"][i])) and np.array_equal(_bits(og["info_vec"][i]), _bits(gg["info_vec"][i])), what


# ------------------------------------------------------------------------------------------------------------ shared, computed once
@pytest.fixture(scope="module")
def ctxs():
    from g2o_frontend_amd import api
    c = {s: api.Context(device=0, max_rows=480, max_cols=640, max_batch=32, omega_storage=s) for s in ("exact9", "sym6")}
    for x in c.values():
        x.set_profiling(True)
    yield c
    for x in c.values():
        x.close()


@pytest.fixture
def oracle_gaussians(oracle):
    """the oracle computes Gaussians inside convert while this is on; switched back off whatever happens"""
    oracle.set_gaussians(True, BASELINE, ALPHA)
    try:
        yield oracle
    finally:
        oracle.set_gaussians(False)


def unscaled_pool(rows, cols, kind):
    """POOL frames of the noise and pattern kinds of tests/depth_frames.py (no NaN, overflow or edge-value frames)"""
    b = DF.make_batch(rows, cols, kind, "kinect", n=2 * DF.MAX_FRAMES, seed=11)
    keep = [i for i, k in enumerate(b.kinds) if k.startswith("noise") or k.split("_odd")[0] in DF.PATTERNS][:POOL]
    assert len(keep) == POOL
    return [np.ascontiguousarray(b.frames[i]) for i in keep]


def scaled_pool(oracle, cfg, kind):
    raw = S.raw_pool(cfg)
    if kind == "raw":
        return [np.ascontiguousarray(f) for f in raw]
    return [oracle.convert_16u_to_32f(f, S.RAW_SCALE) for f in raw]      # room and ladder frames (no signs frames)


def params_for(oracle, shape, step, offset):
    if step:
        (rows, cols) = shape
        K = S.camera(rows, cols)
        K = tuple(F(v) / F(step) for v in K)
        return oracle.converter_params(K=K, sensor_offset=offset, **oracle.QVGA4_CONF_CONVERTER)
    return DF.converter_params(oracle, "kinect", sensor_offset=offset)


def run_shape(ctxs, oracle, shape, step, counts):
    """every variant of one shape: element type x memory x sensor offset x storage, each with one of the frame counts, dealt so that every count
    meets every element type and both memories over the shapes; the per-frame route is computed once per (type, offset, storage)"""
    from g2o_frontend_amd import api
    rows, cols = shape
    orows, ocols = (rows // step, cols // step) if step else (rows, cols)
    k = UNSCALED.index(shape) if not step else len(UNSCALED) + SCALED.index((shape, step))
    v = 0
    for kind in ("float", "raw"):
        raw_scale = None if kind == "float" else (S.RAW_SCALE if step else DF.CONFIGS["kinect"]["scale"])
        pool = scaled_pool(oracle, (shape, step), kind)[:max(counts)] if step else unscaled_pool(rows, cols, kind)[:max(counts)]
        for with_offset in (False, True):
            p = params_for(oracle, shape, step, sensor_offset() if with_offset else None)
            for storage in ("exact9", "sym6"):
                ctx = ctxs[storage]
                images = float_images(ctx, pool, raw_scale, step)
                want = []
                for i, img in enumerate(images):
                    c = per_frame(ctx, p, img)
                    if storage == "exact9":
                        same_as_oracle(oracle.convert(p, oracle.depth_scale(oracle.convert_16u_to_32f(pool[i], raw_scale) if kind == "raw" else pool[i], step, COV)
                                                      if step else (oracle.convert_16u_to_32f(pool[i], raw_scale) if kind == "raw" else pool[i]))[0], c,
                                       (shape, step, kind, with_offset, i))
                    want.append(snapshot(c))
                    del c
                for where in ("device", "host"):
                    n = counts[(k + v) % len(counts)]
                    v += 1
                    frames = pool[:n]
                    buf = ctx.upload(np.stack(frames)) if where == "device" else None
                    args = [buf.frame(i) for i in range(n)] if buf is not None else [np.array(f, copy=True) for f in frames]
                    clouds = [api.Cloud(ctx, orows * ocols) for _ in range(n)]
                    rc = batch_ex(ctx, p, args, raw_scale, rows, cols, step, clouds, extras())
                    assert rc == OK, (shape, step, kind, where, with_offset, storage, n, ctx._L.pwn_hip_last_error_string(ctx.h))
                    nsub = 1      # max_batch 32 >= 25 frames: one sub-batch, one Gaussian launch
                    assert ctx.stage_ms("gaussians")[1] == nsub
                    bad = [(i, differing(want[i], snapshot(c))) for i, c in enumerate(clouds) if differing(want[i], snapshot(c))]
                    assert not bad, (shape, step, kind, where, with_offset, storage, n, bad[:3])
                    assert all(c.numGaussians() == c.size() for c in clouds)
                    del clouds
                    if buf is not None:
                        buf.free()


# ------------------------------------------------------------------------------------------- against the per-frame route and the oracle
@pytest.mark.parametrize("shape", UNSCALED, ids=["%dx%d" % s for s in UNSCALED])
def test_unscaled_batches_equal_the_per_frame_route_and_the_oracle(ctxs, oracle_gaussians, shape):
    run_shape(ctxs, oracle_gaussians, shape, 0, COUNTS)


@pytest.mark.parametrize("cfg", SCALED, ids=[S.config_id(c) for c in SCALED])
def test_scaled_batches_equal_the_per_frame_route_and_the_oracle(ctxs, oracle_gaussians, cfg):
    shape, step = cfg
    run_shape(ctxs, oracle_gaussians, shape, step, (3,) if shape == (480, 640) else COUNTS)


def test_the_two_store_forms_write_the_same_bits(ctxs, oracle):
    """k_gaussians_batch with every lane storing its own record, and staged through LDS: the same clouds, partial last block included"""
    from g2o_frontend_amd import api
    ctx = ctxs["exact9"]
    rows, cols = 17, 129
    pool = unscaled_pool(rows, cols, "raw")[:17]
    p = params_for(oracle, (rows, cols), 0, sensor_offset())
    got = {}
    try:
        for form in (0, 1):
            ctx.check(ctx._L.pwn_hip_debug_set_gaussian_stores(ctx.h, form))
            clouds = [api.Cloud(ctx, rows * cols) for _ in pool]
            assert batch_ex(ctx, p, pool, 0.001, rows, cols, 0, clouds, extras()) == OK
            got[form] = [snapshot(c) for c in clouds]
    finally:
        ctx.check(ctx._L.pwn_hip_debug_set_gaussian_stores(ctx.h, -1))
    assert all(not differing(a, b) for a, b in zip(got[0], got[1]))
    assert sum(s["size"] for s in got[0]) > 0


# ---------------------------------------------------------------------------------------------------------- no extras means no change
@pytest.mark.parametrize("step", [0, 2])
@pytest.mark.parametrize("kind", ["float", "raw"])
def test_no_extras_is_the_existing_call(ctxs, oracle, kind, step):
    from g2o_frontend_amd import api
    ctx = ctxs["sym6"]
    shape = (34, 136) if step else (65, 130)
    rows, cols = shape
    orows, ocols = (rows // step, cols // step) if step else shape
    raw_scale = None if kind == "float" else 0.001
    pool = (scaled_pool(oracle, (shape, step), kind) if step else unscaled_pool(rows, cols, kind))[:17]
    p = params_for(oracle, shape, step, None)
    n = len(pool)
    old = [api.Cloud(ctx, orows * ocols) for _ in range(n)]
    assert existing_call(ctx, p, pool, raw_scale, rows, cols, step, old) == OK
    stages_old = {s: ctx.stage_ms(s)[1] for s in STAGES}
    want = [flat_bytes(c) for c in old]
    assert stages_old["gaussians"] == 0 and stages_old["stats"] == 1
    for ex in (None, extras(0, 0, 0.0, 0.0), extras(0, 0)):
        new = [api.Cloud(ctx, orows * ocols) for _ in range(n)]
        assert batch_ex(ctx, p, pool, raw_scale, rows, cols, step, new, ex) == OK
        assert {s: ctx.stage_ms(s)[1] for s in STAGES} == stages_old
        assert [flat_bytes(c) for c in new] == want
        assert [c.size() for c in new] == [c.size() for c in old]
        assert all(c.numGaussians() == 0 and not has_stats(c) for c in new)
    # each extra alone: Stats without Gaussians, Gaussians without Stats; the core arrays stay those of the lean call
    for ks, ga in ((1, 0), (0, 1)):
        new = [api.Cloud(ctx, orows * ocols) for _ in range(n)]
        assert batch_ex(ctx, p, pool, raw_scale, rows, cols, step, new, extras(ks, ga)) == OK
        assert [flat_bytes(c) for c in new] == want
        assert all(has_stats(c) == bool(ks) and c.numGaussians() == (c.size() if ga else 0) for c in new)


# -------------------------------------------------------------------------------------------------------- slot reuse and sub-batches
def test_slot_reuse_and_sub_batches_on_two_streams(oracle):
    from g2o_frontend_amd import api
    shape, step = (34, 136), 2
    rows, cols = shape
    orows, ocols = rows // step, cols // step
    p = params_for(oracle, shape, step, sensor_offset())
    frames = [S.room(rows, cols, 100 + s) for s in range(13)]      # 13 frames from 13 seeds
    ref_ctx = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=8, omega_storage="exact9")
    small = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=4, omega_storage="exact9")
    two = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=8, omega_storage="exact9")
    try:
        want = [snapshot(per_frame(ref_ctx, p, img)) for img in float_images(ref_ctx, frames, S.RAW_SCALE, step)]
        # a context of 4 slots takes 9 scaled frames: 4 + 4 + 1 through the same slots
        small.set_profiling(True)
        clouds = [api.Cloud(small, orows * ocols) for _ in range(9)]
        dev = small.upload(np.stack(frames[:9]))
        assert batch_ex(small, p, [dev.frame(i) for i in range(9)], S.RAW_SCALE, rows, cols, step, clouds, extras()) == OK
        assert small.stage_ms("gaussians")[1] == 3
        assert [i for i, c in enumerate(clouds) if differing(want[i], snapshot(c))] == []
        # 13 frames as 4 + 4 + 4 + 1 on two streams, host frames through the copy stream; twice, the same bits
        two.set_subbatch(4, 4); two.set_concurrency(2); two.set_profiling(True)
        runs = []
        for _ in range(2):
            clouds = [api.Cloud(two, orows * ocols) for _ in range(13)]
            assert batch_ex(two, p, [np.array(f, copy=True) for f in frames], S.RAW_SCALE, rows, cols, step, clouds, extras()) == OK
            assert two.stage_ms("gaussians")[1] == 4
            runs.append([snapshot(c) for c in clouds])
        assert sum(1 for i in range(13) if differing(want[i], runs[0][i])) == 0
        assert sum(1 for i in range(13) if differing(runs[0][i], runs[1][i])) == 0
        del clouds
    finally:
        for c in (ref_ctx, small, two):
            c.close()


# --------------------------------------------------------------------------------------------------------------- content transitions
def test_content_transitions(ctxs, oracle, tmp_path):
    from g2o_frontend_amd import api
    ctx = ctxs["exact9"]
    rows, cols = 65, 130
    N = rows * cols
    pool = unscaled_pool(rows, cols, "float")[:2]
    p = params_for(oracle, (rows, cols), 0, None)
    rng = np.random.default_rng(5)

    def records(n):
        return (rng.standard_normal((n, 3)).astype(F), rng.standard_normal((n, 9)).astype(F), rng.standard_normal((n, 3)).astype(F),
                rng.standard_normal((n, 9)).astype(F), rng.integers(0, 4, n).astype(np.int32))
    # a cloud that held 500 Gaussians, converted without the option: none
    c = api.Cloud(ctx, N)
    c.debugSetGaussians(*records(500))
    assert c.numGaussians() == 500
    assert existing_call(ctx, p, pool[:1], None, rows, cols, 0, [c]) == OK
    assert c.numGaussians() == 0 and c.size() > 0
    c.debugSetGaussians(*records(500))
    assert batch_ex(ctx, p, pool[:1], None, rows, cols, 0, [c], extras(1, 0)) == OK
    assert c.numGaussians() == 0 and has_stats(c)
    # capacity above the size: the count is the size, the records beyond it are not written
    cap = N + 300
    big = api.Cloud(ctx, cap)
    fill = records(cap)
    big.debugSetGaussians(*fill)
    assert batch_ex(ctx, p, pool[:1], None, rows, cols, 0, [big], extras()) == OK
    n = big.size()
    assert 0 < n < N and big.numGaussians() == n
    inside = big.gaussians()
    big.debugExposeGaussians(cap)
    after = big.gaussians()
    for k, a in zip(GAUSS_KEYS, fill):
        assert np.array_equal(_bits(after[k][n:]), _bits(a[n:])), k
        assert np.array_equal(_bits(after[k][:n]), _bits(inside[k])), k
    assert not np.array_equal(after["flags"][:n], fill[4][:n])
    big.debugExposeGaussians(n)
    # a batch cloud with Stats saves the file the per-frame route's cloud saves
    ref = per_frame(ctx, p, pool[1])
    got = api.Cloud(ctx, N)
    assert batch_ex(ctx, p, pool[1:2], None, rows, cols, 0, [got], extras(1, 0)) == OK
    fa, fb = str(tmp_path / "a.pwn"), str(tmp_path / "b.pwn")
    assert ref.save(fa, binary=True) and got.save(fb, binary=True)
    assert open(fa, "rb").read() == open(fb, "rb").read() and os.path.getsize(fa) > 176 * got.size()


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_every_cloud_as_it_was(ctxs, oracle):
    from g2o_frontend_amd import api
    ctx = ctxs["exact9"]
    shape, step = (34, 136), 2
    rows, cols = shape
    orows, ocols = rows // step, cols // step
    p = params_for(oracle, shape, step, None)
    pool = scaled_pool(oracle, (shape, step), "raw")[:3]
    clouds = [api.Cloud(ctx, orows * ocols) for _ in range(3)]
    assert batch_ex(ctx, p, pool, S.RAW_SCALE, rows, cols, step, clouds, extras()) == OK
    before = [state(c) for c in clouds]
    assert all(s[2] and s[3] == s[1] > 0 for s in before)
    other = pool[::-1]      # what an accepted call would have converted instead
    nan, inf = float("nan"), float("inf")
    n = 3
    ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in other])
    handles = (C.c_void_p * n)(*[c.h for c in clouds])
    null_frame = (C.c_void_p * n)(other[0].ctypes.data, None, other[2].ctypes.data)
    null_cloud = (C.c_void_p * n)(clouds[0].h, clouds[1].h, None)
    ctx.set_omega_storage("sym6")
    odd = api.Cloud(ctx, orows * ocols)
    ctx.set_omega_storage("exact9")
    mixed = (C.c_void_p * n)(clouds[0].h, odd.h, clouds[2].h)
    tiny = api.Cloud(ctx, 8)      # fewer points than its frame's valid scaled pixels: refused before any cloud is touched
    tiny_state = state(tiny)
    small = (C.c_void_p * n)(clouds[0].h, clouds[1].h, tiny.h)
    cases = [
        ("baseline nan", INVALID, dict(ex=extras(1, 1, nan, ALPHA))),
        ("alpha inf", INVALID, dict(ex=extras(1, 1, BASELINE, inf))),
        ("alpha nan, flags off", INVALID, dict(ex=extras(0, 0, BASELINE, nan))),
        ("gaussians 2", INVALID, dict(ex=extras(1, 2))),
        ("keep_stats -1", INVALID, dict(ex=extras(-1, 1))),
        ("step -1", INVALID, dict(step=-1)),
        ("empty scaled image", INVALID, dict(step=rows + 1)),
        ("null frame", INVALID, dict(frame_ptrs=null_frame)),
        ("null cloud", INVALID, dict(handles=null_cloud)),
        ("mixed storages", INVALID, dict(handles=mixed)),
        ("frame larger than the context", CAPACITY, dict(rows=481, cols=641)),
        ("cloud too small (scaled)", CAPACITY, dict(handles=small)),
        ("null frame, unscaled", INVALID, dict(step=0, frame_ptrs=null_frame)),
    ]
    for what, status, kw in cases:
        rc = batch_ex(ctx, p, other, S.RAW_SCALE, kw.get("rows", rows), kw.get("cols", cols), kw.get("step", step), clouds, kw.get("ex", extras()),
                      frame_ptrs=kw.get("frame_ptrs", ptrs), handles=kw.get("handles", handles))
        assert rc == status, (what, rc)
        assert ctx._L.pwn_hip_last_error_string(ctx.h), what
        assert [state(c) for c in clouds] == before, what
        assert state(tiny) == tiny_state, what
    # and the accepted call does change them
    assert batch_ex(ctx, p, other, S.RAW_SCALE, rows, cols, step, clouds, extras()) == OK
    assert [state(c) for c in clouds] != before


# ------------------------------------------------------------------------------------------------------------------- the Python mirror
def test_python_mirror_options(oracle):
    """computeBatch, makeCloudBatch, makeCloud (one frame through the new call) and CloudCache.get with the options against compute() per frame"""
    from g2o_frontend_amd import api
    from test_gpu_merge_clouds import Km, converter_for, natural
    case = natural(60, 80, with_offset=True)
    rows, cols, K, off = case["rows"], case["cols"], case["K"], case["offset"]
    ctx = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=4, omega_storage="exact9")
    try:
        converter = converter_for(ctx, case)
        frames = case["frames"][:3]
        want = []
        for f in frames:
            c = api.Cloud(ctx, rows * cols)
            converter.compute(c, f, sensorOffset=off, keep_stats=True, gaussians=True)
            want.append(snapshot(c))
        clouds = [api.Cloud(ctx, rows * cols) for _ in frames]
        converter.computeBatch(clouds, frames, sensorOffset=off, keep_stats=True, gaussians=True)
        assert [differing(w, snapshot(c)) for w, c in zip(want, clouds)] == [[], [], []]
        converter.computeBatch(clouds, frames, sensorOffset=off)                      # and lean again: what the clouds held is gone
        assert all(c.numGaussians() == 0 and not has_stats(c) for c in clouds)
        aligner = api.Aligner(ctx); aligner.setProjector(converter.projector())
        matcher = api.PwnMatcherBase(aligner, converter); matcher.setScale(1)
        made = matcher.makeCloudBatch(Km(K), off, frames, keep_stats=True, gaussians=True)[0]
        one = matcher.makeCloud(Km(K), off, frames[1], keep_stats=True, gaussians=True)[0]
        assert matcher.numCalls == 4
        for w, c in zip(want + [want[1]], made + [one]):
            a, b = dict(w), snapshot(c)
            a.pop("flat"); b.pop("flat")      # makeCloud's clouds are sized r * c as well; the flat form differs only where a capacity would
            assert not differing(a, b)
        lean = matcher.makeCloud(Km(K), off, frames[1])[0]
        assert lean.numGaussians() == 0 and not has_stats(lean) and lean.size() == one.size()
        cache = api.CloudCache(matcher, capacity=4, sceneReady=True)
        for k, f in enumerate(frames):
            cache.addFrame(k, f, Km(K), off)
        got = cache.get(2)                                                              # a miss through makeCloud
        a, b = dict(want[2]), snapshot(got)
        a.pop("flat"); b.pop("flat")
        assert not differing(a, b) and (cache.hits, cache.misses) == (0, 1)
        del clouds, made, one, lean, got, cache
    finally:
        ctx.close()


# ----------------------------------------------------------------------------------------------------------- the flow that was broken
def write_scene_file(path, case, fused, merger):
    a = fused.arrays(stats=True)
    g = fused.gaussians()
    arrays = [a[k] for k in CLOUD_KEYS] + [merger.pesiTot(), np.array(merger.appended, np.int32), np.array(merger.fused, np.int32)] + [g[k] for k in GAUSS_KEYS]
    with open(path, "wb") as f:
        conf = case["conf"]
        f.write(struct.pack("<3i", case["rows"], case["cols"], len(case["frames"])))
        f.write(np.asarray(case["K"], np.float64).tobytes())
        f.write(struct.pack("<2d3i", conf["min_distance"], conf["max_distance"], conf["min_image_radius"], conf["max_image_radius"], conf["min_points"]))
        for fr, pose in zip(case["frames"], case["poses"]):
            f.write(np.asarray(pose, np.float64).tobytes())
            f.write(np.ascontiguousarray(fr, F).tobytes())
        f.write(struct.pack("<2i", fused.size(), fused.numGaussians()))
        for arr in arrays:
            b = np.ascontiguousarray(arr).tobytes()
            f.write(struct.pack("<q", len(b))); f.write(b)


def test_scene_ready_cache_feeds_the_merger(oracle, tmp_path):
    """nine key frames at 120 x 160 along synth.trajectory: CloudCache(sceneReady=True) -> PwnMerger.mergeNodeList -> Merger.merge"""
    from g2o_frontend_amd import api, build
    from test_gpu_merge_clouds import Km, converter_for, natural
    build.build_tools()
    case = natural(120, 160)
    rows, cols, K = case["rows"], case["cols"], case["K"]
    eye = np.eye(4, dtype=F)
    own = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=9, omega_storage="exact9")
    try:
        def objects():
            converter = converter_for(own, case)
            aligner = api.Aligner(own); aligner.setProjector(converter.projector())
            matcher = api.PwnMatcherBase(aligner, converter); matcher.setScale(1)
            return converter, matcher
        nodes = [api.MapNode(k, case["poses"][k]) for k in range(9)]

        def fuse(scene_ready):
            converter, matcher = objects()
            cache = api.CloudCache(matcher, capacity=16, sceneReady=scene_ready)
            for k in range(9):
                cache.addFrame(k, case["frames"][k], Km(K), eye)
            merger = api.Merger2(own, converter, matcher)
            fused = api.PwnMerger(merger, cache).mergeNodeList(nodes[0], nodes)
            assert cache.get(0) is fused
            return fused, merger, cache, converter
        lean, _, _, _ = fuse(False)
        assert lean.numGaussians() == 0 and lean.size() > 0      # today's behaviour
        fused, merger, cache, converter = fuse(True)
        assert fused.numGaussians() == fused.size() > 0
        assert all(cache.get(k).numGaussians() == cache.get(k).size() for k in range(1, 9))
        # the same list from clouds made frame by frame (the scale is 1: the oracle-scaled frame is the frame)
        conv2, matcher2 = objects()
        singles = []
        for fr in case["frames"]:
            c = api.Cloud(own, rows * cols)
            conv2.compute(c, oracle.depth_scale(fr, 1, COV), sensorOffset=eye, keep_stats=True, gaussians=True)
            singles.append(c)
        m2 = api.Merger2(own, conv2, matcher2)
        m2.mergeBatch([api.PwnMerger.nodeTransform(nodes[0], o) for o in nodes], eye, singles)
        tot = m2.cloudTot()
        assert merger.appended == m2.appended and merger.fused == m2.fused
        a, b = snapshot(fused), snapshot(tot)
        a.pop("flat"); b.pop("flat")      # the capacities differ (the fused cloud is exact-sized), the arrays must not
        assert not differing(a, b), differing(a, b)
        assert np.array_equal(merger.pesiTot(), m2.pesiTot())
        # the C++ mirror, before the clouds are merged in place
        path = str(tmp_path / "scene.bin")
        write_scene_file(path, case, fused, merger)
        r = subprocess.run([os.path.join(ROOT, "tools", "pwn_hip_scene_ready_check"), path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        # Merger::merge takes the fused cloud, and gives what it gives on the per-frame-built total
        out = []
        for cloud, conv in ((fused, converter), (tot, conv2)):
            mg = api.Merger()
            mg.setDepthImageConverter(conv); mg.setImageSize(rows, cols)
            kept = mg.merge(cloud, eye)
            out.append((kept, mg.collapsedIndices().tobytes(), snapshot(cloud)))
        assert out[0][0] == out[1][0] > 0 and out[0][1] == out[1][1]
        x, y = out[0][2], out[1][2]
        x.pop("flat"); y.pop("flat")
        assert not differing(x, y), differing(x, y)
        # the lean cloud cannot be handed to Merger::merge
        from g2o_frontend_amd import _lib
        mg = api.Merger(); mg.setDepthImageConverter(converter); mg.setImageSize(rows, cols)
        with pytest.raises(_lib.PwnHipError):
            mg.merge(lean, eye)
        del fused, tot, lean, cache, merger, m2, singles
    finally:
        own.close()
