"""The grouped storage of the integral image (pwn_kernels.h: ig_at) that the lean converter paths keep between the front end and k_stats: three
interleaved arrays (x y z n) (xx xy xz yy) (yz zz) instead of ten planes.  Nothing outside the library sees the layout, so the check is
end to end: the same frames through a lean call (computeBatch: grouped) and, frame by frame, through the non-lean pwn_hip_convert (ten
planes) must give the same bits in every array of the cloud and in the stored index image.
  * 17 frames: k_unproject_integral_grouped -> k_stats (single pass from 16 frames on), two full XCD groups and a ragged one;
  *  9 frames: k_unproject_integral_rows -> k_integral_cols -> k_stats with the XCD-aware placement and a ragged group;
  *  2 frames: the same producers, frame-major k_stats grid;
  *  the fused step on 9 pairs (18 frames) against computeBatch + alignBatchRecords.
All comparisons are bitwise: the layout moves values, it computes nothing."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import case_params

gpu = pytest.mark.gpu

# 16 x 64: one band, one strip; 37 x 53: partial band, partial strip, an odd pixel count (every second workspace slot starts 8 bytes off a
# 16-byte boundary); 33 x 130: three strips, the last 2 columns wide, so the 16-byte rows end unaligned to the strip; 120 x 160
SIZES = [(16, 64), (37, 53), (33, 130), (120, 160)]
KINDS = ("scene", "invalid", "single", "checker", "near", "far")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_frames(rows, cols):
    """uint16 millimetre frames, one per kind, then three more scenes (9 in all).  With the 120 x 160 configuration (fx = 131.25, world radius
    0.1 m, image radius 3..6): the near plane at 0.6 m asks for radius 21 -> max_image_radius, windows reach all four borders; the far plane at
    4.4 m asks for 2 -> min_image_radius."""
    from g2o_frontend_amd import synth
    K = (131.25, 131.25, (cols - 1) / 2.0, (rows - 1) / 2.0)
    out = []
    for kind in KINDS:
        if kind == "scene":
            f = synth.render_depth_mm(11, None, rows, cols, K)
        elif kind == "invalid":
            f = np.zeros((rows, cols), np.uint16)
        elif kind == "single":
            f = np.zeros((rows, cols), np.uint16); f[rows // 2, cols // 3] = 1500
        elif kind == "checker":
            f = synth.render_depth_mm(12, None, rows, cols, K, holes=0.0)
            v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
            f[(u + v) % 2 == 1] = 0
        elif kind == "near":
            f = np.full((rows, cols), 600, np.uint16)
        else:
            f = np.full((rows, cols), 4400, np.uint16)
        out.append(np.ascontiguousarray(f))
    for seed in (13, 14, 15):
        out.append(np.ascontiguousarray(synth.render_depth_mm(seed, None, rows, cols, K, holes=0.1)))
    return K, out


def converter_for(K, rows, cols):
    from g2o_frontend_amd import api
    _, _, _, conv, _ = case_params("small")
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    proj.setMinDistance(conv["min_distance"]); proj.setMaxDistance(conv["max_distance"]); proj.setImageSize(rows, cols)
    stats = api.StatsCalculatorIntegralImage()
    stats.setWorldRadius(conv["world_radius"]); stats.setMinImageRadius(conv["min_image_radius"]); stats.setMaxImageRadius(conv["max_image_radius"])
    stats.setMinPoints(conv["min_points"]); stats.setCurvatureThreshold(conv["stats_curvature_threshold"])
    pinfo, ninfo = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
    pinfo.setCurvatureThreshold(conv["point_info_curvature_threshold"]); ninfo.setCurvatureThreshold(conv["normal_info_curvature_threshold"])
    return api.DepthImageConverterIntegralImage(proj, stats, pinfo, ninfo)


def stored_index(cloud):
    """the index image the cloud keeps, read from its flat form (pwn_hip_cloud_export)"""
    buf = np.zeros(cloud.flatSize(), np.uint8)
    assert cloud.exportFlat(buf) == buf.size
    b = buf.tobytes()
    valid, rows, cols = struct.unpack_from("<iii", b, 20)
    assert valid == 1
    off, = struct.unpack_from("<Q", b, 184)
    return np.frombuffer(b, np.int32, rows * cols, off).reshape(rows, cols)


class Rig:
    """context, converter, frames and the non-lean results (ten planes) of one (size, storage): computed once, left unchanged"""
    def __init__(self, rows, cols, storage):
        from g2o_frontend_amd import api
        self.rows, self.cols = rows, cols
        self.ctx = api.Context(0, rows, cols, 32, omega_storage=storage)
        self.ctx.set_profiling(True)
        self.K, self.raw = make_frames(rows, cols)
        self.conv = converter_for(self.K, rows, cols)
        self.depth = [self.ctx.DepthImage_convert_16UC1_to_32FC1(f, 0.001) for f in self.raw]
        self.want = []
        for d in self.depth:
            cloud = api.Cloud(self.ctx, rows * cols)
            self.conv.compute(cloud, d)                     # index and interval image out: the non-lean path
            assert self.ctx.stage_ms("integral_rows")[1] == 1
            self.want.append((cloud.arrays(), self.conv.indexImage().copy()))
        normals = sum(int((np.abs(a["normals"][:, :3]).sum(1) > 0).sum()) for a, _ in self.want)
        assert normals > rows * cols, "degenerate input: no normals to compare"

    def check_batch(self, order, single_pass, raw):
        from g2o_frontend_amd import api
        clouds = [api.Cloud(self.ctx, self.rows * self.cols) for _ in order]
        frames = [self.raw[i] if raw else self.depth[i] for i in order]
        self.conv.computeBatch(clouds, frames, raw_scale=0.001 if raw else None)
        ran = {s: self.ctx.stage_ms(s)[1] for s in ("integral", "integral_rows", "integral_cols", "stats")}
        assert ran == (dict(integral=1, integral_rows=0, integral_cols=0, stats=1) if single_pass else dict(integral=0, integral_rows=1, integral_cols=1, stats=1)), ran
        for j, (i, cloud) in enumerate(zip(order, clouds)):
            a, idx = self.want[i]
            g = cloud.arrays()
            for k in ("points", "normals", "curvature", "omega_p", "omega_n"):
                assert a[k].shape == g[k].shape and np.array_equal(_bits(a[k]), _bits(g[k])), (self.rows, self.cols, len(order), raw, j, KINDS[i] if i < len(KINDS) else i, k)
            assert np.array_equal(idx, stored_index(cloud)), (self.rows, self.cols, len(order), raw, j, i)


_RIGS = {}


@pytest.fixture(scope="module")
def rigs():
    def get(rows, cols, storage):
        if (rows, cols, storage) not in _RIGS:
            _RIGS[(rows, cols, storage)] = Rig(rows, cols, storage)
        return _RIGS[(rows, cols, storage)]
    yield get
    for r in _RIGS.values():
        r.ctx.close()
    _RIGS.clear()


@gpu
@pytest.mark.parametrize("storage", ["exact9", "sym6"])
@pytest.mark.parametrize("shape", SIZES, ids=[f"{r}x{c}" for r, c in SIZES])
def test_lean_batch_of_9_equals_non_lean_frame_by_frame(rigs, shape, storage):
    """9 frames (one more than a multiple of 8): the row / column producers write the grouped image, k_stats reads it with the XCD placement"""
    rig = rigs(*shape, storage)
    rig.check_batch(list(range(9)), single_pass=False, raw=False)
    rig.check_batch(list(range(9)), single_pass=False, raw=True)


@gpu
@pytest.mark.parametrize("storage", ["exact9", "sym6"])
@pytest.mark.parametrize("shape", SIZES, ids=[f"{r}x{c}" for r, c in SIZES])
def test_lean_batch_of_17_equals_non_lean_frame_by_frame(rigs, shape, storage):
    """17 frames: the single-pass strip kernel stores the grouped image with 16-byte and 8-byte rows; every kind of frame lands in an even and in
    an odd workspace slot"""
    rig = rigs(*shape, storage)
    order = [j % 9 for j in range(17)]
    assert {(i, j % 2) for j, i in enumerate(order)} >= {(i, p) for i in range(len(KINDS)) for p in (0, 1)}
    rig.check_batch(order, single_pass=True, raw=False)
    rig.check_batch(order, single_pass=True, raw=True)


@gpu
@pytest.mark.parametrize("storage", ["exact9", "sym6"])
@pytest.mark.parametrize("shape", [(37, 53), (120, 160)], ids=["37x53", "120x160"])
def test_two_frames_equal_non_lean_frame_by_frame(rigs, shape, storage):
    """under 8 frames: the latency-path producers and the frame-major k_stats grid; every kind of frame in slot 0 and in slot 1"""
    rig = rigs(*shape, storage)
    for a in range(0, 6, 2):
        rig.check_batch([a, a + 1], single_pass=False, raw=False)
        rig.check_batch([a + 1, a], single_pass=False, raw=True)
    rig.check_batch([0, 8], single_pass=False, raw=True)


@gpu
def test_fused_step_of_9_pairs_equals_convert_then_align():
    """convertAlignBatch on 9 pairs at 120 x 160 (18 frames, single pass): the records of computeBatch + alignBatchRecords, bit for bit"""
    from g2o_frontend_amd import api, shard, synth
    from test_gpu_parity import gpu_objects
    n = 9
    rows, cols, K, _, _ = case_params("small")
    ctx = api.Context(0, rows, cols, 32, omega_storage="sym6")
    _, converter, aligner = gpu_objects(ctx, "small")
    pairs = [synth.make_pair(7100 + s, rows, cols, K) for s in range(n)]
    rf = [p[0] for p in pairs]; cf = [p[1] for p in pairs]
    refs = [api.Cloud(ctx, rows * cols) for _ in range(n)]; curs = [api.Cloud(ctx, rows * cols) for _ in range(n)]
    converter.computeBatch(refs + curs, rf + cf, raw_scale=0.001)
    ids = np.arange(300, 300 + n, dtype=np.int32)
    want = np.full((n, shard.RECORD_FLOATS), -5.0, np.float32)
    aligner.alignBatchRecords(refs, curs, want, pair_ids=ids)
    refs2 = [api.Cloud(ctx, rows * cols) for _ in range(n)]; curs2 = [api.Cloud(ctx, rows * cols) for _ in range(n)]
    rec = np.full((n, shard.RECORD_FLOATS), -7.0, np.float32)
    aligner.convertAlignBatch(converter, refs2, curs2, rf, cf, raw_scale=0.001, records=rec, pair_ids=ids)
    assert (want[:, 62] > 0).all(), "no iterations ran: nothing compared"
    assert np.array_equal(_bits(rec), _bits(want))
    ctx.close()


def test_grouped_strip_kernel_stores_whole_records_and_no_packed_xyz():
    """k_unproject_integral_grouped is a kernel of its own because it stores 16-byte rows, which the strip kernel that also stores the 12-byte
    point records must not contain (test_capi_cpu.py).  It writes no 12-byte record at all -- nothing a widened store could run over -- its
    plane stores are the 16-byte and 8-byte rows of the y pass, and it spills nothing."""
    from g2o_frontend_amd import _lib
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf not installed")
    blob = open(_lib.LIB_PATH, "rb").read()
    i = blob.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert i >= 0
    n = struct.unpack_from("<Q", blob, i + 24)[0]; off = i + 32
    code = None
    for _ in range(n):
        o, sz, tl = struct.unpack_from("<QQQ", blob, off); name = blob[off + 24: off + 24 + tl].decode(); off += 24 + tl
        if "gfx950" in name:
            code = blob[i + o: i + o + sz]
    assert code, "no gfx950 code object in the library"
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code); f.flush()
        asm = subprocess.run([objdump, "-d", f.name], capture_output=True, text=True).stdout
        notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
    counts, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1); continue
        m = re.search(r"\b(global|flat)_(store|load)_dword(x\d)?\b", line)
        if m and cur and "28k_unproject_integral_groupedE" in cur:
            counts[m.group(0)] = counts.get(m.group(0), 0) + 1
    kIR_Rows = 8
    assert counts.get("global_store_dwordx4") == kIR_Rows, counts          # one 16-byte store per row of the band (groups 0 and 1 share the code)
    assert counts.get("global_store_dwordx2", 0) >= kIR_Rows, counts       # group 2's rows (and the hand-over word)
    assert "global_store_dwordx3" not in counts and not any(k.startswith("flat_") for k in counts), counts
    m = re.search(r"\.name:\s+\S*28k_unproject_integral_groupedE\S*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s*(\d+)", notes)
    assert m and int(m.group(1)) == 0, m and m.group(0)
