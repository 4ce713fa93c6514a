"""The fused pass's strip index: in the one-call step (pwn_hip_convert_align_batch_u16) a sub-batch that takes the depth source
(tests/test_gpu_cur_from_depth.py), whose width is a multiple of 64 and whose current frames were converted by the single-pass strip front end
(launches of at least 16 frames) runs k_corr_linearize without loading the current index image either: a pixel's index is the word of its
64-column strip in the table of strip offsets the converter left with the cloud, plus the pixel's rank among the strip's valid depths.

The yardstick is the stored-index, stored-point path: the split route (pwn_hip_convert_batch_u16, then pwn_hip_align_batch_records).  Step and
split route run on different clouds and must agree bit for bit in the records, the result fields, the step traces and every byte of the clouds
afterwards (flat form).  pwn_hip_debug_strip_index_sub_batches says which path ran.

Shapes and contents: tests/strip_index_frames.py.  The small shapes run as many pairs in one sub-batch as the throughput shape takes; most
pairs are seeded natural frames, and one pair per content family has that family's frame as its current frame.
"""
import ctypes as C

import numpy as np
import pytest

import cur_depth_frames as F
import strip_index_frames as S
from test_gpu_cur_from_depth import OFFSET, Rig, guesses, same, throughput_pairs

pytestmark = pytest.mark.gpu

MIN_FRAMES = 16      # launches of at least this many frames take the single-pass strip front end


class StripRig(Rig):
    def pairs(self, n, seed, families=True):
        """n (reference, current) frames on the device: a few seeded natural pairs in turn; the first len(S.FAMILIES) pairs take a family's frame
        as their current frame"""
        host = [F.make_pair(seed + s, self.rows, self.cols) for s in range(3)]
        fam = [S.frame(k, self.rows, self.cols, seed) for k in S.FAMILIES] if families else []
        dref = [self.ctx.upload(r) for r, _ in host]; dcur = [self.ctx.upload(c) for _, c in host]; dfam = [self.ctx.upload(f) for f in fam]
        self.bufs += dref + dcur + dfam
        rf = [dref[i % 3] for i in range(n)]
        cf = [dfam[i] if i < len(dfam) else dcur[i % 3] for i in range(n)]
        return rf, cf

    def strips(self):
        k = C.c_int(-1)
        self.ctx.check(self.ctx._L.pwn_hip_debug_strip_index_sub_batches(self.ctx.h, C.byref(k)))
        return k.value


def pairs_for(rows, cols):
    return max(throughput_pairs(rows, cols), MIN_FRAMES)


def one_sub_batch(rows, cols, n, omega="sym6"):
    rig = StripRig(rows, cols, n, omega)
    rig.ctx.set_subbatch(n, n); rig.ctx.set_concurrency(1)
    return rig


@pytest.mark.parametrize("rows,cols", S.SHAPES[:3])
@pytest.mark.parametrize("omega", ["sym6", "exact9"])
def test_small_shapes_identity_and_other_guesses(rows, cols, omega):
    """one sub-batch in the throughput shape: identity guesses, then a second step on the same clouds with other frames and non-identity guesses
    (the table is the new conversion's)"""
    n = pairs_for(rows, cols)
    rig = one_sub_batch(rows, cols, n, omega)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    for seed, g in ((7, None), (40, guesses(n))):
        rf, cf = rig.pairs(n, seed)
        a = rig.step(refs, curs, rf, cf, guess=g)
        assert (a[3], rig.strips()) == (1, 1)
        assert (a[0]["iter_correspondences"][len(S.FAMILIES):, 0] > 0).any(), "degenerate input"
        b = rig.split(refs2, curs2, rf, cf, guess=g)
        assert (b[3], rig.strips()) == (0, 0)
        same(a, b, refs + curs, refs2 + curs2)
    rig.close()


def test_vga_once():
    rows, cols, n = 480, 640, MIN_FRAMES
    rig = one_sub_batch(rows, cols, n)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    rf, cf = rig.pairs(n, 11)
    g = guesses(n); g[1] = np.eye(4, dtype=np.float32); g[9] = np.eye(4, dtype=np.float32)
    a = rig.step(refs, curs, rf, cf, guess=g)
    assert (a[3], rig.strips()) == (1, 1)
    assert (a[0]["iter_inliers"][len(S.FAMILIES):, 0] > 0).all(), "degenerate input"
    b = rig.split(refs2, curs2, rf, cf, guess=g)
    assert (b[3], rig.strips()) == (0, 0)
    same(a, b, refs + curs, refs2 + curs2)
    rig.close()


def test_uneven_sub_batches_on_two_streams():
    """190 pairs of 40 x 128 with sub_pairs 100: sub-batches of 100 and 90 pairs on two streams, both in the throughput shape, both converted in
    launches of 100 resp. 90 frames"""
    rows, cols, n, sub = 40, 128, 190, 100
    rig = StripRig(rows, cols, 2 * sub)
    rig.ctx.set_subbatch(sub, sub); rig.ctx.set_concurrency(2)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    rf, cf = rig.pairs(n, 19)
    g = guesses(n)
    a = rig.step(refs, curs, rf, cf, guess=g)
    assert (a[3], rig.strips()) == (2, 2)
    b = rig.split(refs2, curs2, rf, cf, guess=g)
    assert (b[3], rig.strips()) == (0, 0)
    same(a, b, refs + curs, refs2 + curs2)
    rig.close()


def test_small_conversion_launches_keep_the_index_image():
    """sub_frames 8: the step converts in launches of 8 frames, the three-kernel front end, whose offsets are per row -- the depth source stays, the
    index is loaded"""
    rows, cols = 30, 320
    n = pairs_for(rows, cols)
    rig = StripRig(rows, cols, n)
    rig.ctx.set_subbatch(8, n); rig.ctx.set_concurrency(1)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    rf, cf = rig.pairs(n, 23)
    a = rig.step(refs, curs, rf, cf)
    assert (a[3], rig.strips()) == (1, 0)
    b = rig.split(refs2, curs2, rf, cf)
    same(a, b, refs + curs, refs2 + curs2)
    rig.close()


@pytest.mark.parametrize("rows,cols", S.FALLBACK_SHAPES)
def test_other_widths_keep_the_index_image(rows, cols):
    n = pairs_for(rows, cols)
    rig = one_sub_batch(rows, cols, n)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    rf, cf = rig.pairs(n, 7)
    a = rig.step(refs, curs, rf, cf)
    assert (a[3], rig.strips()) == (1, 0)
    b = rig.split(refs2, curs2, rf, cf)
    same(a, b, refs + curs, refs2 + curs2)
    rig.close()


def test_converter_sensor_offset_keeps_the_stored_index():
    rows, cols = 40, 128
    n = pairs_for(rows, cols)
    rig = one_sub_batch(rows, cols, n)
    rig.aligner.setSensorOffset(OFFSET)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    rf, cf = rig.pairs(n, 7)
    a = rig.step(refs, curs, rf, cf, offset=OFFSET)
    assert (a[3], rig.strips()) == (0, 0)
    b = rig.split(refs2, curs2, rf, cf, offset=OFFSET)
    same(a, b, refs + curs, refs2 + curs2)
    rig.close()


def test_scaled_step_and_host_frames_keep_the_stored_index():
    """80 x 256 frames at half resolution (40 x 128, a width that would qualify), and a step on host frames: no depth source, no strip index"""
    from g2o_frontend_amd import api, shard, synth
    from test_gpu_scaled_batch import COV, OK, make_aligner, make_converter, scaled_call
    rows, cols, step = 80, 256, 2
    n = pairs_for(rows // step, cols // step)
    rig = StripRig(rows, cols, n)
    Ks = synth.scaled_K(F.camera(rows, cols), step)
    rig.converter = make_converter(Ks)
    rig.aligner = make_aligner(rig.ctx, Ks, rows // step, cols // step)
    rig.ctx.set_subbatch(n, n); rig.ctx.set_concurrency(1)
    N = (rows // step) * (cols // step)
    mk = lambda: [api.Cloud(rig.ctx, N) for _ in range(n)]      # noqa: E731
    refs, curs, refs2, curs2 = mk(), mk(), mk(), mk()
    rf, cf = rig.pairs(n, 23, families=False)
    a = rig.step(refs, curs, rf, cf, step=step, max_depth_cov=COV)
    assert (a[3], rig.strips()) == (0, 0)
    assert scaled_call(rig.ctx, rig.converter.params(None), "raw", rf + cf, rows, cols, step, refs2 + curs2) == OK
    rec = np.full((n, shard.RECORD_FLOATS), -7.0, np.float32)
    got = rig.aligner.alignBatchRecords(refs2, curs2, rec, pair_ids=np.arange(50, 50 + n, dtype=np.int32)).copy()
    same(a, (got, rec, rig.ctx.last_align_steps(0, n), 0), refs + curs, refs2 + curs2)
    rig.close()
    rows, cols = 40, 128
    n = pairs_for(rows, cols)
    rig = one_sub_batch(rows, cols, n)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    host = [F.make_pair(7 + s, rows, cols) for s in range(3)]
    rf = [host[i % 3][0] for i in range(n)]; cf = [host[i % 3][1] for i in range(n)]
    a = rig.step(refs, curs, rf, cf)
    assert (a[3], rig.strips()) == (0, 0)
    b = rig.split(refs2, curs2, rf, cf)
    same(a, b, refs + curs, refs2 + curs2)
    rig.close()


def test_imported_current_clouds_have_no_table():
    """clouds that went through their flat form carry the index image but no strip offsets: aligned on their own, and as the targets of a later
    step (whose conversion gives them a table of their own)"""
    from test_gpu_scaled_batch import flat_bytes
    rows, cols = 40, 128
    n = pairs_for(rows, cols)
    rig = one_sub_batch(rows, cols, n)
    refs, curs, refs2, curs2 = rig.clouds(n), rig.clouds(n), rig.clouds(n), rig.clouds(n)
    rf, cf = rig.pairs(n, 7)
    a = rig.step(refs, curs, rf, cf)
    assert (a[3], rig.strips()) == (1, 1)
    for src, dst in zip(curs, curs2):
        dst.importFlat(flat_bytes(src))
    for src, dst in zip(refs, refs2):
        dst.importFlat(flat_bytes(src))
    from g2o_frontend_amd import shard
    rec = np.full((n, shard.RECORD_FLOATS), -7.0, np.float32)
    got = rig.aligner.alignBatchRecords(refs2, curs2, rec, pair_ids=np.arange(50, 50 + n, dtype=np.int32)).copy()
    assert (rig.counter(), rig.strips()) == (0, 0)
    same(a, (got, rec, rig.ctx.last_align_steps(0, n), 0), refs + curs, refs2 + curs2)
    rf, cf = rig.pairs(n, 31)
    a = rig.step(refs2, curs2, rf, cf)
    assert (a[3], rig.strips()) == (1, 1)
    b = rig.split(refs, curs, rf, cf)
    same(a, b, refs2 + curs2, refs + curs)
    rig.close()


def test_capacity_below_the_valid_count():
    """Current clouds that hold fewer points than their frames have valid pixels: the step reports the capacity error after its kernels have run,
    and its records are written.  Indices at or above the capacity drop out of the pass -- from the table and the ballot exactly as from the
    stored index image (the same step with conversion launches of 8 frames, which loads it)."""
    from g2o_frontend_amd import _lib, api, shard
    rows, cols = 30, 320
    n = pairs_for(rows, cols)
    cap = rows * cols // 3
    recs = []
    for sub_frames, want in ((n, 1), (8, 0)):
        rig = StripRig(rows, cols, n)
        rig.ctx.set_subbatch(sub_frames, n); rig.ctx.set_concurrency(1)
        refs = rig.clouds(n); curs = [api.Cloud(rig.ctx, cap) for _ in range(n)]
        rf, cf = rig.pairs(n, 7, families=False)
        rec = np.full((n, shard.RECORD_FLOATS), -7.0, np.float32)
        prepared = rig.aligner.convertAlignHandles(refs, curs, rf, cf)[:6] + ((rig.converter.params(None), rig.aligner.params()),)
        with pytest.raises(_lib.PwnHipError):
            rig.aligner.convertAlignBatch(rig.converter, None, None, None, None, raw_scale=F.SCALE, records=rec,
                                          pair_ids=np.arange(50, 50 + n, dtype=np.int32), prepared=prepared)
        assert (rig.counter(), rig.strips()) == (1, want)
        assert (rec != -7.0).any(), "the records were not written"
        recs.append(rec)
        rig.close()
    assert np.array_equal(recs[0].view(np.uint32), recs[1].view(np.uint32))
