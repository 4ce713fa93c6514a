"""The traversability image on the GPU: pwn_hip_manifold_image against the numpy model of ManifoldVoronoiExtractor::process
(tests/manifold_image.py), image and per-cloud inside counts bit for bit, on injected and natural clouds; host, device and misaligned device
images; both omega storages, uploaded and converter-made clouds; accumulation, split calls and the chunked path; the two mirrors; refusals.
Every comparison is of integers."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_image as M      # noqa: E402
import merge_clouds as MC      # noqa: E402
from conftest import case_params      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID, CAPACITY = 1, 6
# grid -> clouds in the list; n = 1, 2, 7, 30, 31.  The sort covers the cell ids 0 .. cells (the last one for the points that make no event): one radix
# pass up to 255 cells (1 x 1, 1 x 7, 7 x 1 and 15 x 17, the largest such grid, with the events of seven clouds), two from 256 cells (16 x 16) to
# 65 535 (17 x 16, 37 x 53, 100 x 100), three at 257 x 256; four only at 2^24 cells, see the test of the largest grid
GRIDS = [(1, 1, 1), (1, 7, 2), (7, 1, 7), (15, 17, 7), (16, 16, 7), (17, 16, 30), (37, 53, 31), (100, 100, 7), (257, 256, 2)]


@pytest.fixture(scope="module")
def ctx():
    from g2o_frontend_amd import api
    c = api.Context(device=0, max_rows=120, max_cols=160, max_batch=9, omega_storage="exact9")
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx6():
    from g2o_frontend_amd import api
    c = api.Context(device=0, max_rows=120, max_cols=160, max_batch=9, omega_storage="sym6")
    yield c
    c.close()


def ptr(x):
    from g2o_frontend_amd import api
    return api._ptr(x)


def colmajor(T):
    return np.ascontiguousarray(np.asarray(T, F).T).reshape(-1)


def upload(ctx, a):
    from g2o_frontend_amd import api
    n = len(a["points"])
    c = api.Cloud(ctx, max(1, n))
    if n:
        c.upload(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])
    return c


def call(ctx, clouds, transforms, resolution, xs, ys, image, accumulate=0, thr=M.THR, counts=True):
    """pwn_hip_manifold_image -> (status, inside[n]); image (numpy uint16, a DeviceBuffer or a raw address) is written in place"""
    n = len(clouds)
    handles = (C.c_void_p * max(1, n))(*[c.h for c in clouds])
    tr = np.ascontiguousarray(np.stack([colmajor(T) for T in transforms]), F) if n else np.zeros((1, 16), F)
    inside = (C.c_int * max(1, n))(*([-7] * max(1, n)))
    p = image if isinstance(image, C.c_void_p) else ptr(image)
    rc = ctx._L.pwn_hip_manifold_image(ctx.h, n, handles, ptr(tr), resolution, xs, ys, thr, accumulate, p, inside if counts else None)
    return rc, np.array(list(inside)[:n], np.int32)


def uploaded_injected(ctx, xs, ys, n):
    case, rows = M.injected(xs, ys, 0.2, n)
    return case, rows, [upload(ctx, a) for a in case["arrays"]]


# --------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("xs,ys,n", GRIDS)
def test_injected_clouds_bit_exact(ctx, oracle, xs, ys, n):
    case, rows, clouds = uploaded_injected(ctx, xs, ys, n)
    want, winside, events, longest = M.splat(rows, 0.2, xs, ys)
    img = np.full((xs, ys), 7, np.uint16)
    rc, inside = call(ctx, clouds, case["transforms"], 0.2, xs, ys, img)
    assert rc == 0
    print("%d x %d, %d clouds: %d events, largest run %d, %d cells differ" % (xs, ys, n, events, longest, int((img != want).sum())))
    assert np.array_equal(inside, winside), (inside, winside)
    assert np.array_equal(img, want)


def natural_converted(ctx, case, n):
    from test_gpu_merge_clouds import natural_on_gpu
    return natural_on_gpu(ctx, case, n)


@pytest.mark.parametrize("resolution", [0.05, 0.2])
def test_natural_frames_bit_exact(ctx, ctx6, oracle, resolution):
    case, trs, rows = M.natural()
    want, winside, events, longest = M.splat(rows, resolution, 100, 100)
    obstacles, heights = int((want == M.OBSTACLE).sum()), int(((want != M.OBSTACLE) & (want != M.UNTOUCHED)).sum())
    print("resolution %.2f: %d obstacle cells, %d height cells, %d events, largest run %d" % (resolution, obstacles, heights, events, longest))
    for c, made in ((ctx, "uploaded"), (ctx, "converted"), (ctx6, "uploaded"), (ctx6, "converted")):
        clouds = [upload(c, o.arrays()) for o in case["clouds"]] if made == "uploaded" else natural_converted(c, case, 9)
        img = np.zeros((100, 100), np.uint16)
        rc, inside = call(c, clouds, trs, resolution, 100, 100, img)
        assert rc == 0 and np.array_equal(inside, winside) and np.array_equal(img, want), (made, c is ctx6, int((img != want).sum()))


def test_converter_made_clouds_at_120_x_160(ctx, ctx6, oracle):
    case = MC.natural_case(120, 160, case_params("small")[2], n=3, with_offset=True)
    trs = M.relative_transforms(case["poses"], 2)
    rows = [M.transformed(c, T) for c, T in zip(case["clouds"], trs)]
    want, winside, _, _ = M.splat(rows, 0.05, 100, 100)
    for c in (ctx, ctx6):
        img = np.zeros((100, 100), np.uint16)
        rc, inside = call(c, natural_converted(c, case, 3), trs, 0.05, 100, 100, img)
        assert rc == 0 and np.array_equal(inside, winside) and np.array_equal(img, want)


def test_empty_outside_and_repeated_clouds(ctx, oracle):
    case, rows, clouds = uploaded_injected(ctx, 37, 53, 31)
    far = {k: v.copy() for k, v in case["arrays"][3].items()}
    far["points"][:, 0] += F(1000)                        # wholly outside the grid
    empty = {k: v[:0] for k, v in far.items()}
    eye = M.EYE
    lst = [clouds[0], upload(ctx, empty), upload(ctx, far), clouds[0], clouds[5]]
    trs = [eye, eye, eye, eye, case["transforms"][5]]
    mrows = [rows[0], (np.zeros((0, 3), F), np.zeros((0, 3), F)), M.transformed(M.oracle_cloud(far), eye), rows[0], rows[5]]
    want, winside, _, _ = M.splat(mrows, 0.2, 37, 53)
    assert winside[1] == 0 and winside[2] == 0 and winside[0] == winside[3] > 0
    img = np.zeros((37, 53), np.uint16)
    rc, inside = call(ctx, lst, trs, 0.2, 37, 53, img)
    assert rc == 0 and np.array_equal(inside, winside) and np.array_equal(img, want)
    # n == 0 fills the image, or leaves it under accumulate
    img[:] = 5
    assert call(ctx, [], [], 0.2, 37, 53, img)[0] == 0 and (img == M.UNTOUCHED).all()
    img[:] = 5
    assert call(ctx, [], [], 0.2, 37, 53, img, accumulate=1)[0] == 0 and (img == 5).all()


def test_the_largest_grid_keeps_a_cells_good_and_bad_events_in_one_run(oracle):
    """4096 x 4096 is the largest grid the call takes: 2^24 cells, so the cell of the points that make no event is 2^24 and the sort runs four passes,
    over all of the key's low word.  The bad flag must lie above it, or the last pass parts a cell's bad events from its good ones.  Cells at the
    corners, in the middle and with every byte of the cell id in use get, in turn, (good 9000, bad 8000) -> obstacle and (good 8000, bad 9000) -> 8000,
    within one cloud and across two; seen alone, the good events miss the first and the bad events miss the second."""
    from g2o_frontend_amd import api
    size = 4096
    c, ires = size // 2, F(1)
    at = [(0, 0), (0, 4095), (4095, 0), (4095, 4095), (2048, 2048), (1, 255), (255, 256), (16, 1), (4095, 4094), (3003, 1717), (17, 4095), (2047, 2049)]
    up, side = np.array([0, 0, 1], F), np.array([1, 0, 0], F)
    first, second = [], []          # (point, normal) of cloud 0 and cloud 1
    for k, (x, y) in enumerate(at):
        px, py = M.coordinate_for(x, c, ires), M.coordinate_for(y, c, ires)
        good, bad = (9000, 8000) if k % 2 == 0 else (8000, 9000)
        first.append(((px, py, M.z_for_pz(good)), up))
        (first if k % 4 < 2 else second).append(((px, py, M.z_for_pz(bad)), side))
        first.append(((F(5000), py, F(0)), up))                   # outside the grid
        second.append(((px, py, F(9)), np.zeros(3, F)))           # no normal: no event
    arrays = [M.cloud_arrays(np.array([p for p, _ in lst], F), np.array([n for _, n in lst], F)) for lst in (first, second)]
    rows = [M.transformed(M.oracle_cloud(a), M.EYE) for a in arrays]
    want, winside, events, longest = M.splat(rows, 1.0, size, size)
    assert events == 2 * len(at) and longest == 2
    for k, (x, y) in enumerate(at):
        assert want[x, y] == (M.OBSTACLE if k % 2 == 0 else 8000), (x, y)
    assert int((want != M.UNTOUCHED).sum()) == len(at)
    own = api.Context(device=0, max_rows=16, max_cols=16, max_batch=1)
    try:
        clouds = [upload(own, a) for a in arrays]
        dev = api.DeviceBuffer(own, np.zeros(size * size, np.uint16))      # 32 MB
        rc, inside = call(own, clouds, [M.EYE, M.EYE], 1.0, size, size, dev)
        got = dev.numpy().reshape(size, size)
        print("4096 x 4096: %d events, %d cells differ" % (events, int((got != want).sum())))
        assert rc == 0 and np.array_equal(inside, winside)
        assert np.array_equal(got, want), [(x, y, int(got[x, y]), int(want[x, y])) for x, y in at]
        del clouds, dev
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------- pointer variants of `image`
def test_host_device_and_misaligned_device_images(ctx, oracle):
    from g2o_frontend_amd import api
    xs, ys = 37, 53
    case, rows, clouds = uploaded_injected(ctx, xs, ys, 31)
    want, winside, _, _ = M.splat(rows, 0.2, xs, ys)
    cells = xs * ys
    host = np.full(cells + 32, 0xABCD, np.uint16)         # pageable, sentinels on both sides
    rc, inside = call(ctx, clouds, case["transforms"], 0.2, xs, ys, host[16:16 + cells])
    assert rc == 0 and np.array_equal(host[16:16 + cells].reshape(xs, ys), want) and (host[:16] == 0xABCD).all() and (host[16 + cells:] == 0xABCD).all()
    for lead in (16, 9):                                  # a 16-byte boundary of the allocation, and one element behind one
        dev = api.DeviceBuffer(ctx, np.full(cells + 32, 0xABCD, np.uint16))
        assert dev.data_ptr() % 16 == 0
        rc, inside = call(ctx, clouds, case["transforms"], 0.2, xs, ys, C.c_void_p(dev.data_ptr() + 2 * lead), counts=(lead == 16))
        got = dev.numpy()
        assert rc == 0 and np.array_equal(got[lead:lead + cells].reshape(xs, ys), want), lead
        assert (got[:lead] == 0xABCD).all() and (got[lead + cells:] == 0xABCD).all(), lead
        if lead == 16:
            assert np.array_equal(inside, winside)


# ------------------------------------------------------------------------------------------------- accumulation and chunking
def test_split_calls_prefilled_images_and_the_chunked_path(ctx, oracle):
    xs, ys = 37, 53
    case, rows, clouds = uploaded_injected(ctx, xs, ys, 31)
    trs = case["transforms"]
    want8 = M.splat(rows[:8], 0.2, xs, ys)[0]
    one = np.zeros((xs, ys), np.uint16)
    assert call(ctx, clouds[:8], trs[:8], 0.2, xs, ys, one)[0] == 0 and np.array_equal(one, want8)
    two = np.zeros((xs, ys), np.uint16)
    assert call(ctx, clouds[:3], trs[:3], 0.2, xs, ys, two)[0] == 0
    assert call(ctx, clouds[3:8], trs[3:8], 0.2, xs, ys, two, accumulate=1)[0] == 0
    assert np.array_equal(two, one)
    # a pre-filled image: the walk starts from what it holds (host and device)
    from g2o_frontend_amd import api
    rng = np.random.default_rng(5)
    start = rng.choice(np.array([30000, 65535, 9000, 9300, 12000, 0, 65436], np.uint16), (xs, ys))
    wantp, winside, _, _ = M.splat(rows, 0.2, xs, ys, image=start)
    img = start.copy()
    rc, inside = call(ctx, clouds, trs, 0.2, xs, ys, img, accumulate=1)
    assert rc == 0 and np.array_equal(img, wantp) and np.array_equal(inside, winside)
    dev = api.DeviceBuffer(ctx, start)
    assert call(ctx, clouds, trs, 0.2, xs, ys, dev, accumulate=1)[0] == 0 and np.array_equal(dev.numpy(), wantp)
    # chunks of whole clouds with at most 8 192 points (the largest cloud fits, two of the seeded ones of 4 097 do not): the same bits
    want, winside, _, _ = M.splat(rows, 0.2, xs, ys)
    assert max(len(P) for P, _ in rows) <= 8192 < sum(len(P) for P, _ in rows)
    try:
        assert ctx._L.pwn_hip_debug_set_manifold_chunk(ctx.h, 8192) == 0
        img = np.zeros((xs, ys), np.uint16)
        rc, inside = call(ctx, clouds, trs, 0.2, xs, ys, img)
        assert rc == 0 and np.array_equal(img, want) and np.array_equal(inside, winside)
        # a cloud above the bound is refused, nothing written
        assert ctx._L.pwn_hip_debug_set_manifold_chunk(ctx.h, 4096) == 0
        img[:] = 5
        rc, inside = call(ctx, clouds, trs, 0.2, xs, ys, img)
        assert rc == CAPACITY and (img == 5).all() and (inside == -7).all()
    finally:
        assert ctx._L.pwn_hip_debug_set_manifold_chunk(ctx.h, 0) == 0


# ---------------------------------------------------------------------------------------------------------------- the mirrors
def Km(K):
    return np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], F)


def test_mirrors_push_key_nodes_one_at_a_time(oracle, tmp_path):
    from g2o_frontend_amd import api, build
    from test_gpu_merge_clouds import converter_for
    build.build_tools()
    case, _, _ = M.natural()
    rows, cols, K, conf = case["rows"], case["cols"], case["K"], case["conf"]
    own = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=9, omega_storage="exact9")
    try:
        converter = converter_for(own, case)
        aligner = api.Aligner(own); aligner.setProjector(converter.projector())
        matcher = api.PwnMatcherBase(aligner, converter); matcher.setScale(1)
        cache = api.CloudCache(matcher, capacity=16)
        nodes = [api.MapNode(k, case["poses"][k]) for k in range(9)]
        for k in range(9):
            cache.addFrame(k, case["frames"][k], Km(K), case["offset"])
        ex = api.ManifoldVoronoiExtractor(cache)
        ex.setQueueSize(3); ex.setResolution(0.05)
        records = []
        for k in range(9):
            d = ex.process(nodes[k])
            assert d.node is nodes[k] and d.resolution == 0.05 and d.image.shape == (100, 100) and d.image.dtype == np.uint16
            records.append((list(ex.inside), d.image.copy()))
        # the last record is the direct call on the last three clouds, and the model on the oracle's conversions of them
        last = [cache.get(k) for k in (6, 7, 8)]
        trs = M.relative_transforms(case["poses"], 8)[6:]
        img = np.zeros((100, 100), np.uint16)
        rc, inside = call(own, last, trs, 0.05, 100, 100, img)
        assert rc == 0 and np.array_equal(img, records[-1][1]) and inside.tolist() == records[-1][0]
        want, winside, _, _ = M.splat([M.transformed(c, T) for c, T in zip(case["clouds"][6:], trs)], 0.05, 100, 100)
        assert np.array_equal(img, want) and np.array_equal(inside, winside)
        assert [len(r[0]) for r in records] == [1, 2, 3, 3, 3, 3, 3, 3, 3]
        path = str(tmp_path / "manifold.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<3i", rows, cols, 9))
            f.write(np.asarray(K, np.float64).tobytes())
            f.write(struct.pack("<2d3i", conf["min_distance"], conf["max_distance"], conf["min_image_radius"], conf["max_image_radius"], conf["min_points"]))
            f.write(np.ascontiguousarray(case["offset"], F).tobytes())
            f.write(struct.pack("<3i2f", 100, 100, 3, 0.05, M.THR))
            for fr, p in zip(case["frames"], case["poses"]):
                f.write(np.asarray(p, np.float64).tobytes()); f.write(np.ascontiguousarray(fr, F).tobytes())
            for ins, im in records:
                f.write(struct.pack("<i", len(ins))); f.write(np.array(ins, np.int32).tobytes()); f.write(np.ascontiguousarray(im).tobytes())
        r = subprocess.run([os.path.join(ROOT, "tools", "pwn_hip_manifold_check"), path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        del last, cache, ex
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_image_and_the_counts_untouched(ctx, oracle):
    from g2o_frontend_amd import api
    xs, ys = 37, 53
    case, rows, clouds = uploaded_injected(ctx, xs, ys, 31)
    L = ctx._L
    other = api.Context(device=0, max_rows=16, max_cols=16, max_batch=1)
    foreign = api.Cloud(other, 16)
    host = np.full((xs, ys), 5, np.uint16)
    dev = api.DeviceBuffer(ctx, host)
    inside = (C.c_int * 2)(-3, -3)
    tr = np.ascontiguousarray(np.stack([colmajor(M.EYE)] * 2))
    h = lambda *cl: (C.c_void_p * 2)(*[x.h if x is not None else None for x in cl])      # noqa: E731
    ok = h(clouds[0], clouds[1])
    for image in (host, dev):
        def args(ctxh=ctx.h, n=2, cl=ok, t=ptr(tr), res=0.2, x=xs, y=ys, img=ptr(image)):
            return (ctxh, n, cl, t, res, x, y, M.THR, 0, img, inside)
        refused = [(INVALID, args(ctxh=None)), (INVALID, args(cl=None)), (INVALID, args(t=None)), (INVALID, args(img=None)), (INVALID, args(n=-1)),
                   (INVALID, args(cl=h(clouds[0], None))), (INVALID, args(cl=h(clouds[0], foreign))),
                   (INVALID, args(x=0)), (INVALID, args(y=0)), (INVALID, args(x=-3)), (INVALID, args(x=4097, y=4096)),
                   (INVALID, args(res=0.0)), (INVALID, args(res=-0.2)), (INVALID, args(res=float("inf"))), (INVALID, args(res=float("nan")))]
        for want, a in refused:
            assert L.pwn_hip_manifold_image(*a) == want, a
        assert L.pwn_hip_last_error_string(ctx.h)
    assert list(inside) == [-3, -3] and (host == 5).all() and (dev.numpy() == 5).all()
    # and the call still works afterwards
    rc, ins = call(ctx, clouds[:2], case["transforms"][:2], 0.2, xs, ys, host)
    want, winside, _, _ = M.splat(rows[:2], 0.2, xs, ys)
    assert rc == 0 and np.array_equal(host, want) and np.array_equal(ins, winside)
    del foreign
    other.close()
