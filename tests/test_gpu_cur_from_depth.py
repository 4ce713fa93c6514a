"""The fused pass's depth source: in the one-call step (pwn_hip_convert_align_batch_u16) a sub-batch whose pairs all take the current cloud's own
index image, whose frames are the caller's resident uint16 frames and which is large enough for the throughput shape of k_corr_linearize runs
that kernel without loading the current points -- each is recomputed from the raw depth of its pixel (pwn_math.h converter_point).

The yardstick is the stored-point path: the split route (pwn_hip_convert_batch_u16, then pwn_hip_align_batch_records) never has a depth source.
Step and split route run on different clouds and must agree bit for bit in the records, the result fields (pose, and the chi2 / inlier /
correspondence / candidate traces of every iteration), the step traces, and every byte of the clouds afterwards (flat form: all arrays, the
index image and its key).  pwn_hip_debug_cur_depth_sub_batches says which path ran: > 0 in the step, 0 in the split route.

Shapes (tests/cur_depth_frames.py): 24 x 32 (cols < 256: a thread's 256-pixel stride crosses eight rows; one partial 2048-pixel tile),
120 x 160 (cols < 256, N no multiple of 2048), 60 x 300 (cols > 256 and no multiple of it), 480 x 640.  The depth source belongs to the
throughput shape (more workgroups in a launch than the device has compute units; smaller launches take k_corr_linearize_lat and the stored
points), so the small shapes run as many pairs in one sub-batch as that takes; the pairs cycle through a few seeded frames.
"""
import ctypes as C

import numpy as np
import pytest

import cur_depth_frames as F

pytestmark = pytest.mark.gpu

FIELDS = ("T", "chi2", "iter_inliers", "iter_correspondences", "iter_candidates", "error", "inliers", "iterations", "n_reference", "n_current")
OFFSET = np.array([[0.0, 0.0, 1.0, 0.1], [-1.0, 0.0, 0.0, 0.05], [0.0, -1.0, 0.0, 0.6], [0.0, 0.0, 0.0, 1.0]], np.float32)
COMPUTE_UNITS = 256      # MI355X


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if np.asarray(a).dtype == np.float32 else np.asarray(a)


def throughput_pairs(rows, cols):
    """pairs a sub-batch needs for the throughput shape: tiles x pairs > compute units"""
    tiles = (rows * cols + 2047) // 2048
    return COMPUTE_UNITS // tiles + 2


def guesses(n):
    """small non-identity initial transforms, one per pair"""
    from g2o_frontend_amd import synth
    return [synth.v2t(np.array([0.01 * ((i % 3) - 1), 0.008, -0.006 * (i % 2), 0.004, -0.003 * (i % 4), 0.002])).astype(np.float32) for i in range(n)]


class Rig:
    def __init__(self, rows, cols, max_batch, omega="sym6"):
        from g2o_frontend_amd import api
        from test_gpu_scaled_batch import make_aligner, make_converter
        self.rows, self.cols = rows, cols
        self.ctx = api.Context(0, rows, cols, max_batch, omega_storage=omega)
        conv, alig = F.configuration(rows, cols)
        K = F.camera(rows, cols)
        self.converter = make_converter(K)
        self.converter._stats.setMinImageRadius(conv["min_image_radius"]); self.converter._stats.setMaxImageRadius(conv["max_image_radius"])
        self.converter._stats.setMinPoints(conv["min_points"])
        self.aligner = make_aligner(self.ctx, K, rows, cols)
        self.aligner.correspondenceFinder().setInlierDistanceThreshold(alig["inlier_distance_threshold"])
        self.bufs = []

    def frames(self, n, seed, distinct=4):
        """n (reference, current) frame pairs on the device, cycling through `distinct` seeded pairs"""
        host = [F.make_pair(seed + s, self.rows, self.cols) for s in range(min(n, distinct))]
        dev = [(self.ctx.upload(r), self.ctx.upload(c)) for r, c in host]
        self.bufs += [b for pr in dev for b in pr]
        return [dev[i % len(dev)][0] for i in range(n)], [dev[i % len(dev)][1] for i in range(n)], host

    def clouds(self, n):
        from g2o_frontend_amd import api
        return [api.Cloud(self.ctx, self.rows * self.cols) for _ in range(n)]

    def counter(self):
        k = C.c_int(-1)
        self.ctx.check(self.ctx._L.pwn_hip_debug_cur_depth_sub_batches(self.ctx.h, C.byref(k)))
        return k.value

    def step(self, refs, curs, rf, cf, guess=None, offset=None, **kw):
        """the one-call step -> (results, records, step traces, counter)"""
        from g2o_frontend_amd import shard
        n = len(refs)
        rec = np.full((n, shard.RECORD_FLOATS), -7.0, np.float32)
        prepared = self.aligner.convertAlignHandles(refs, curs, rf, cf)[:6] + ((self.converter.params(offset), self.aligner.params()),)
        if "step" in kw:
            prepared += ((kw["step"], kw["max_depth_cov"]),)
        got = self.aligner.convertAlignBatch(self.converter, None, None, None, None, raw_scale=F.SCALE, records=rec, pair_ids=np.arange(50, 50 + n, dtype=np.int32),
                                             initialGuesses=guess, prepared=prepared).copy()
        return got, rec, self.ctx.last_align_steps(0, n), self.counter()

    def split(self, refs, curs, rf, cf, guess=None, offset=None):
        """convert, wait, align: the stored-point path"""
        from g2o_frontend_amd import shard
        n = len(refs)
        self.converter.computeBatch(refs + curs, rf + cf, sensorOffset=offset, raw_scale=F.SCALE)
        rec = np.full((n, shard.RECORD_FLOATS), -7.0, np.float32)
        got = self.aligner.alignBatchRecords(refs, curs, rec, pair_ids=np.arange(50, 50 + n, dtype=np.int32), initialGuesses=guess).copy()
        return got, rec, self.ctx.last_align_steps(0, n), self.counter()

    def close(self):
        for b in self.bufs:
            b.free()
        self.ctx.close()


def same(a, b, clouds_a, clouds_b):
    """results, records, step traces and clouds of two routes, bit for bit"""
    from test_gpu_scaled_batch import flat_bytes
    (ga, ra, sa, _), (gb, rb, sb, _) = a, b
    for k in FIELDS:
        assert np.array_equal(_bits(ga[k]), _bits(gb[k])), k
    assert np.array_equal(_bits(ra), _bits(rb))
    for x, y in zip(sa, sb):
        assert x["iterations"] == y["iterations"] and x["converged"] == y["converged"]
        assert np.array_equal(_bits(x["step_translation"]), _bits(y["step_translation"])) and np.array_equal(_bits(x["step_rotation"]), _bits(y["step_rotation"]))
    for x, y in zip(clouds_a, clouds_b):
        assert np.array_equal(flat_bytes(x), flat_bytes(y))


def nontrivial(got):
    assert (got["iterations"] == 10).all() and (got["iter_correspondences"][:, 0] > 0).all() and (got["iter_inliers"][:, 0] > 0).all(), "degenerate input"


@pytest.mark.parametrize("rows,cols", F.SHAPES[:3])
@pytest.mark.parametrize("omega", ["sym6", "exact9"])
def test_small_shapes_identity_and_other_guesses(rows, cols, omega):
    """one sub-batch in the throughput shape: identity guesses (the reference side takes its own index image in iteration 0 as well), then a second
    step on the same clouds with other frames and non-identity guesses (no stale frame pointer; the current index stays the cloud's own)"""
    n = throughput_pairs(rows, cols)
    rig = Rig(rows, cols, n, omega)
    rig.ctx.set_subbatch(n, n); rig.ctx.set_concurrency(1)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    rf, cf, _ = rig.frames(n, 7)
    a = rig.step(refs, curs, rf, cf)
    assert a[3] == 1, a[3]
    nontrivial(a[0])
    b = rig.split(refs2, curs2, rf, cf)
    assert b[3] == 0
    same(a, b, refs + curs, refs2 + curs2)
    rf, cf, _ = rig.frames(n, 40, distinct=3)
    g = guesses(n)
    a = rig.step(refs, curs, rf, cf, guess=g)
    assert a[3] == 1, a[3]
    nontrivial(a[0])
    b = rig.split(refs2, curs2, rf, cf, guess=g)
    assert b[3] == 0
    same(a, b, refs + curs, refs2 + curs2)
    rig.close()


def test_vga_uneven_sub_batches_and_early_stop():
    """5 VGA pairs with sub_pairs 2: sub-batches of 2, 2 and 1 pair on two streams -- two pairs are 300 workgroups (throughput shape, depth source),
    the last pair alone takes the latency shape and the stored points.  Then the same with "stop when converged" on, one loose setting."""
    n = 5
    rig = Rig(480, 640, 8)
    rig.ctx.set_subbatch(4, 2); rig.ctx.set_concurrency(2)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    rf, cf, _ = rig.frames(n, 11, distinct=5)
    g = guesses(n); g[1] = np.eye(4, dtype=np.float32); g[4] = np.eye(4, dtype=np.float32)
    a = rig.step(refs, curs, rf, cf, guess=g)
    assert a[3] == 2, a[3]
    nontrivial(a[0])
    b = rig.split(refs2, curs2, rf, cf, guess=g)
    assert b[3] == 0
    same(a, b, refs + curs, refs2 + curs2)
    rig.ctx.set_convergence(2e-3, 2e-3, 2)
    a = rig.step(refs, curs, rf, cf, guess=g)
    assert a[3] == 2, a[3]
    assert any(s["converged"] and s["iterations"] < 10 for s in a[2]), [s["iterations"] for s in a[2]]
    b = rig.split(refs2, curs2, rf, cf, guess=g)
    assert b[3] == 0
    same(a, b, refs + curs, refs2 + curs2)
    rig.close()


def test_converter_sensor_offset_keeps_the_stored_points():
    """A converter sensor offset moves the points off their pixels: the converter promises no index image, the current clouds are projected, and
    no sub-batch takes the depth source.  Results equal the split route's."""
    rows, cols = 120, 160
    n = throughput_pairs(rows, cols)
    rig = Rig(rows, cols, n)
    rig.ctx.set_subbatch(n, n); rig.ctx.set_concurrency(1)
    rig.aligner.setSensorOffset(OFFSET)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    rf, cf, _ = rig.frames(n, 7)
    a = rig.step(refs, curs, rf, cf, offset=OFFSET)
    assert a[3] == 0, a[3]
    nontrivial(a[0])
    b = rig.split(refs2, curs2, rf, cf, offset=OFFSET)
    assert b[3] == 0
    same(a, b, refs + curs, refs2 + curs2)
    rig.close()


def test_scaled_step_and_host_frames_keep_the_stored_points():
    """The _scaled step converts from a down-sampled temporary whose slot is reused, and a step on host frames from a staging slot: neither passes a
    depth source.  8 VGA pairs at half resolution in one sub-batch (304 workgroups: the throughput shape) against their own split route."""
    from g2o_frontend_amd import api, synth
    from test_gpu_scaled_batch import COV, OK, make_aligner, make_converter, scaled_call
    rows, cols, step, n = 480, 640, 2, 8
    rig = Rig(rows, cols, 16)
    Ks = synth.scaled_K(synth.K_VGA, step)
    rig.converter = make_converter(Ks)
    rig.aligner = make_aligner(rig.ctx, Ks, rows // step, cols // step)
    rig.ctx.set_subbatch(16, 8); rig.ctx.set_concurrency(1)
    N = (rows // step) * (cols // step)
    mk = lambda: [api.Cloud(rig.ctx, N) for _ in range(n)]      # noqa: E731
    refs, curs, refs2, curs2 = mk(), mk(), mk(), mk()
    rf, cf, host = rig.frames(n, 23)
    a = rig.step(refs, curs, rf, cf, step=step, max_depth_cov=COV)
    assert a[3] == 0, a[3]
    nontrivial(a[0])
    from g2o_frontend_amd import shard
    assert scaled_call(rig.ctx, rig.converter.params(None), "raw", rf + cf, rows, cols, step, refs2 + curs2) == OK
    rec = np.full((n, shard.RECORD_FLOATS), -7.0, np.float32)
    got = rig.aligner.alignBatchRecords(refs2, curs2, rec, pair_ids=np.arange(50, 50 + n, dtype=np.int32)).copy()
    b = (got, rec, rig.ctx.last_align_steps(0, n), rig.counter())
    assert b[3] == 0
    same(a, b, refs + curs, refs2 + curs2)
    rig.close()
    # host frames, full resolution, the throughput shape
    rows, cols = 120, 160
    n = throughput_pairs(rows, cols)
    rig = Rig(rows, cols, n)
    rig.ctx.set_subbatch(n, n); rig.ctx.set_concurrency(1)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    host = [F.make_pair(7 + s, rows, cols) for s in range(4)]
    rf = [host[i % 4][0] for i in range(n)]; cf = [host[i % 4][1] for i in range(n)]
    a = rig.step(refs, curs, rf, cf)
    assert a[3] == 0, a[3]
    b = rig.split(refs2, curs2, rf, cf)
    same(a, b, refs + curs, refs2 + curs2)
    rig.close()
