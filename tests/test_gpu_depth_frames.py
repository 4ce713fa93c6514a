"""The converter's front end as shipped (k_row_count / k_strip_count<RAW> / k_strip_count_any, k_row_offsets, k_unproject_integral_rows +
k_integral_cols, k_unproject_integral) through pwn_hip_debug_front_end on the injected frames of tests/depth_frames.py: everything it writes
-- index image, offsets, the ten integral planes, with lean = 0 the points and the interval image -- against the oracle bit for bit, the planes
against float64, stale hand-over words across calls of different shapes and paths, and the same frames through the public convert calls.  With
lean = 2 the same through the grouped kernels every lean convert call launches (k_unproject_integral_grouped, the grouped write-out of
k_unproject_integral_rows, the grouped mode of k_integral_cols)."""
import numpy as np
import pytest

import depth_frames as D

pytestmark = pytest.mark.gpu

PLAN = D.batch_plan()
STAGES = ("unproject", "integral", "integral_rows", "integral_cols", "stats")       # include/pwn_hip.h: pwn_hip_last_stage_ms
EXPECTED = {D.SINGLE_PASS: dict(unproject=1, integral=1, integral_rows=0, integral_cols=0, stats=0),
            D.LATENCY: dict(unproject=1, integral=0, integral_rows=1, integral_cols=1, stats=0)}


@pytest.fixture(scope="module")
def ctx():
    """one context for every shape: 1040 x 72 pixels hold the largest (1025 x 65, 129 x 513), and a slot of 74880 pixels keeps every staged
    frame 16-byte aligned, so that the width alone chooses the counting kernel for host frames"""
    from g2o_frontend_amd import api
    c = api.Context(device=0, max_rows=1040, max_cols=72, max_batch=D.MAX_FRAMES, omega_storage="exact9")
    c.set_profiling(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def made(oracle):
    """batches and the oracle's results, computed once per (shape, element type) and left unchanged"""
    cache = {}

    def get(rows, cols, kind):
        if (rows, cols, kind) not in cache:
            conf = next(cf for r, c, k, cf in PLAN if (r, c, k) == (rows, cols, kind))
            b = D.make_batch(rows, cols, kind, conf)
            cache[(rows, cols, kind)] = (b, D.reference(oracle, b), D.converter_params(oracle, conf))
        return cache[(rows, cols, kind)]
    return get


def window(n, start):
    return [(start + j) % D.MAX_FRAMES for j in range(n)]


def run_and_compare(ctx, b, ref, p, frames, path, lean, device_offset=None):
    got = D.run_gpu(ctx, p, b, frames, path, lean, device_offset)
    ran = {s: ctx.stage_ms(s)[1] for s in STAGES}
    assert ran == EXPECTED[path], (path, ran)
    bad = D.compare(b, frames, ref, got, path, lean)
    print(f"  {b.rows}x{b.cols} {b.kind} {b.conf_name} path {path} lean {lean} {len(frames)} frames from {frames[0]}: differing elements {bad}")
    assert not any(bad.values()), (b.rows, b.cols, b.kind, path, lean, len(frames), bad)
    return got


@pytest.mark.parametrize("case", range(len(PLAN)), ids=[f"{r}x{c}-{k}-{cf}" for r, c, k, cf in PLAN])
def test_front_end_bit_exact_against_oracle(ctx, made, case):
    """every shape x element type, both paths, lean 0 and 1: index image, offsets, planes; with lean = 0 the points and the interval image outside
    the generator's mask of undefined conversions.  The frame counts and the window of the batch's 25 frames move with the case."""
    rows, cols, kind, _ = PLAN[case]
    b, ref, p = made(rows, cols, kind)
    for lean in (0, 1):
        n_sp = D.SINGLE_PASS_COUNTS[(case + 3 * lean) % len(D.SINGLE_PASS_COUNTS)]
        n_lat = D.LATENCY_COUNTS[(case // 2 + lean) % len(D.LATENCY_COUNTS)]
        run_and_compare(ctx, b, ref, p, window(n_sp, 7 * case + 11 * lean), D.SINGLE_PASS, lean)
        run_and_compare(ctx, b, ref, p, window(n_lat, 5 * case + 13 * lean + 3), D.LATENCY, lean)


@pytest.mark.parametrize("shape", [(17, 129), (65, 130)])
def test_every_frame_count_on_multi_strip_shapes(ctx, made, shape):
    """the 8 * ceil(n / 8) frame decode of the single-pass grid and the frame dimension of the latency grids at every count of the plan, on
    shapes with three strips and three / nine bands (the second: the 8 * ceil(bands / 8) band decode with a padded group)"""
    for kind in ("float", "raw"):
        b, ref, p = made(shape[0], shape[1], kind)
        for k, n in enumerate(D.SINGLE_PASS_COUNTS):
            run_and_compare(ctx, b, ref, p, window(n, 3 * k), D.SINGLE_PASS, (k + (kind == "raw")) % 2)
        for k, n in enumerate(D.LATENCY_COUNTS):
            run_and_compare(ctx, b, ref, p, window(n, 5 * k + 1), D.LATENCY, (k + (kind == "raw")) % 2)


def test_undefined_conversions_only_where_the_generator_put_them(ctx, made):
    """all 25 frames of the batches that hold NaN and overflow pixels, lean = 0: the interval differs from the oracle's at most inside the mask, and
    the mask is exactly the undefined pixels the generator placed.  What each side returns there is recorded in docs/parity.md."""
    seen = {}
    for rows, cols, kind in ((17, 129, "float"), (129, 513, "float"), (9, 68, "raw")):      # NaN only; "tiny": NaN and overflow; raw overflow
        b, ref, p = made(rows, cols, kind)
        und = b.undefined_mask()
        placed = sum(1 for i, pl in enumerate(b.placed) for _, r, c in pl if und[i, r, c])
        assert int(und.sum()) == placed and placed > 0, (rows, cols, kind, int(und.sum()), placed)
        frames = list(range(D.MAX_FRAMES))
        for path in (D.SINGLE_PASS, D.LATENCY):
            got = run_and_compare(ctx, b, ref, p, frames if path == D.SINGLE_PASS else frames[:16], path, 0)
            for j, i in enumerate(frames if path == D.SINGLE_PASS else frames[:16]):
                d = b.depth(i)[und[i]]
                for dv, o, g in zip(d, ref[i]["interval"][und[i]], got["interval"][j][und[i]]):
                    seen.setdefault(("NaN" if np.isnan(dv) else "quotient >= 2^31", int(o), int(g)), 0)
                    seen[("NaN" if np.isnan(dv) else "quotient >= 2^31", int(o), int(g))] += 1
    print("undefined conversions (input, oracle's interval, device's interval): pixels", seen)
    assert {k[0] for k in seen} == {"NaN", "quotient >= 2^31"}


def test_device_planes_against_float64(ctx, made):
    """no oracle in the comparison: the device's planes against float64 sums of the fp32 terms of the device's own points and index image, within
    gamma_n * sum |term|, n = r + c + 1 (depth_frames.float64_ratio) -- the largest shapes, both paths"""
    worst = 0.0
    for rows, cols, kind in ((129, 513, "float"), (1025, 65, "raw"), (128, 512, "raw")):
        b, _, p = made(rows, cols, kind)
        for path, frames in ((D.SINGLE_PASS, window(16, 0)), (D.LATENCY, window(9, 16))):
            got = D.run_gpu(ctx, p, b, frames, path, 0)
            for j in range(len(frames)):
                ratio = D.float64_ratio(got["planes"][j], D.channel_terms(got["index"][j], got["points"][j]))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (rows, cols, kind, path, frames[j], ratio)
    print(f"device planes: worst |plane - sum64| / (gamma_n sum|term|) = {worst:.4f}")


def test_stale_hand_over_words_across_shapes_and_paths(ctx, made):
    """Hand-over words outlive a call and differ from fresh ones only in their epoch.  In one context, all bit-exact: two different batches of one
    shape back to back, a shape with other strip and band counts (its words land on other (strip, band) indices of the same memory), the first
    shape again; then the latency path after the single-pass path and the single-pass path after the latency path on one shape."""
    a, ra, pa = made(17, 129, "float")         # 3 strips x 3 bands
    c, rc, pc = made(128, 512, "raw")          # 8 strips x 16 bands
    run_and_compare(ctx, a, ra, pa, window(16, 0), D.SINGLE_PASS, 1)
    run_and_compare(ctx, a, ra, pa, window(16, 9), D.SINGLE_PASS, 1)
    run_and_compare(ctx, c, rc, pc, window(16, 4), D.SINGLE_PASS, 1)
    run_and_compare(ctx, a, ra, pa, window(17, 5), D.SINGLE_PASS, 0)
    run_and_compare(ctx, c, rc, pc, window(15, 2), D.LATENCY, 0)
    run_and_compare(ctx, a, ra, pa, window(15, 11), D.LATENCY, 1)
    run_and_compare(ctx, a, ra, pa, window(24, 1), D.SINGLE_PASS, 0)
    run_and_compare(ctx, a, ra, pa, window(3, 20), D.LATENCY, 0)
    run_and_compare(ctx, c, rc, pc, window(25, 0), D.SINGLE_PASS, 1)


@pytest.mark.parametrize("kind", ["float", "raw"])
def test_frame_pointer_alignment_chooses_the_counting_kernel(ctx, made, kind):
    """16 x 128 has 16-byte aligned rows for both element types (k_strip_count<RAW>); the same frames in device memory one element behind a
    256-byte boundary take k_strip_count_any for the alignment alone.  Both equal the oracle and so each other, bit for bit."""
    b, ref, p = made(16, 128, kind)
    frames = window(17, 6)
    outs = [run_and_compare(ctx, b, ref, p, frames, D.SINGLE_PASS, 0, off) for off in (None, 0, 1)]
    for o in outs[1:]:
        for key in ("index", "rowoff", "interval"):
            assert np.array_equal(outs[0][key], o[key]), key
        assert D.same_bits(outs[0]["planes"], o["planes"]).all()
    run_and_compare(ctx, b, ref, p, frames[:3], D.LATENCY, 0, 1)


# ------------------------------------------------------------------------------------------------ the grouped form (lean = 2)
# What every lean convert call launches: k_unproject_integral_grouped on the single-pass path, the grouped write-out of k_unproject_integral_rows
# and the grouped mode of k_integral_cols on the latency path.  The hook hands the slot back as stored; depth_frames.grouped_to_planes (the
# layout stated a second time, from the header's sentence) turns it into planes for the oracle.
G = D.LEAN_GROUPED


def _grouped_counts(case):
    return D.SINGLE_PASS_COUNTS[(case + 6) % len(D.SINGLE_PASS_COUNTS)], D.LATENCY_COUNTS[(case // 2 + 2) % len(D.LATENCY_COUNTS)]


assert {1, 7, 8, 9, 16, 17, 25} <= {_grouped_counts(c)[0] for c in range(len(PLAN))} and {1, 3, 15, 16} == {_grouped_counts(c)[1] for c in range(len(PLAN))}


@pytest.mark.parametrize("case", range(len(PLAN)), ids=[f"{r}x{c}-{k}-{cf}" for r, c, k, cf in PLAN])
def test_front_end_grouped_bit_exact_against_oracle(ctx, made, case):
    """every shape x element type, both paths, lean = 2: index image, offsets and the planes read out of the grouped records against the oracle bit
    for bit, the stage counters those of a convert call.  Frame counts and windows move with the case; over the plan the single-pass path meets
    1, 7, 8, 9, 16, 17, 24 and 25 frames, the latency path 1, 3, 15 and 16."""
    rows, cols, kind, _ = PLAN[case]
    b, ref, p = made(rows, cols, kind)
    n_sp, n_lat = _grouped_counts(case)
    run_and_compare(ctx, b, ref, p, window(n_sp, 7 * case + 22), D.SINGLE_PASS, G)
    run_and_compare(ctx, b, ref, p, window(n_lat, 5 * case + 29), D.LATENCY, G)


def test_grouped_planes_against_float64(ctx, made):
    """no oracle in the comparison: the planes read out of the grouped records against float64 sums of the fp32 terms of the device's own points
    and index image (from a lean = 0 call on the same frames: a grouped call stores no points), within gamma_n * sum |term|, n = r + c + 1"""
    worst = 0.0
    for rows, cols, kind in ((129, 513, "float"), (1025, 65, "raw")):
        b, _, p = made(rows, cols, kind)
        for path, frames in ((D.SINGLE_PASS, window(16, 0)), (D.LATENCY, window(9, 16))):
            full = D.run_gpu(ctx, p, b, frames, path, 0)
            got = D.run_gpu(ctx, p, b, frames, path, G)
            assert np.array_equal(full["index"], got["index"])
            for j in range(len(frames)):
                ratio = D.float64_ratio(got["planes"][j], D.channel_terms(got["index"][j], full["points"][j]))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (rows, cols, kind, path, frames[j], ratio)
    print(f"grouped planes: worst |plane - sum64| / (gamma_n sum|term|) = {worst:.4f}")


def test_stale_hand_over_words_across_storage_forms(ctx, made):
    """The y pass of the grouped strip kernel carries four chains per thread where the plane kernel carries three, so its hand-over words need not
    sit where the plane kernel's sit; they outlive a call and differ from fresh ones only in their epoch.  In one context: lean 1, 2, 0, 2 in turn
    on different windows of one shape, on the single-pass and on the latency path, then the same at a shape with other strip and band counts,
    then the first shape's grouped call once more -- all bit-exact."""
    a, ra, pa = made(17, 129, "float")         # 3 strips x 3 bands
    c, rc, pc = made(65, 130, "raw")           # 3 strips x 9 bands
    for b, ref, p in ((a, ra, pa), (c, rc, pc)):
        for k, lean in enumerate((1, G, 0, G)):
            run_and_compare(ctx, b, ref, p, window(16 + k % 2, 6 * k + 1), D.SINGLE_PASS, lean)
        for k, lean in enumerate((1, G, 0, G)):
            run_and_compare(ctx, b, ref, p, window((15, 3, 9, 15)[k], 5 * k + 2), D.LATENCY, lean)
    run_and_compare(ctx, a, ra, pa, window(25, 0), D.SINGLE_PASS, G)
    run_and_compare(ctx, a, ra, pa, window(15, 7), D.LATENCY, G)


@pytest.mark.parametrize("kind", ["float", "raw"])
def test_grouped_front_end_on_device_frames_at_every_alignment(ctx, made, kind):
    """9 x 68 in device memory 0, 1, 2 and 4 elements behind a 256-byte boundary, lean = 2: float rows are 16-byte aligned at 0 and 4 elements
    (k_strip_count) and not at 1 and 2 (k_strip_count_any); raw rows of 68 are never (k_strip_count_any, at byte offsets 0, 2, 4 and 8).  Every
    placement equals the oracle and so the host frames' result, bit for bit."""
    b, ref, p = made(9, 68, kind)
    frames = window(17, 4)
    outs = [run_and_compare(ctx, b, ref, p, frames, D.SINGLE_PASS, G, off) for off in (None, 0, 1, 2, 4)]
    for o in outs[1:]:
        for key in ("index", "rowoff"):
            assert np.array_equal(outs[0][key], o[key]), key
        assert D.same_bits(outs[0]["planes"], o["planes"]).all()
    run_and_compare(ctx, b, ref, p, frames[:3], D.LATENCY, G, 2)


def test_front_end_hook_refuses_an_unknown_lean_value(ctx, made):
    """lean = 3 and -1 are PWN_HIP_ERR_INVALID_ARGUMENT and the output arrays keep what they held"""
    import ctypes as C
    b, _, p = made(9, 68, "float")
    N = b.rows * b.cols
    src = np.ascontiguousarray(b.frames[:1])
    from g2o_frontend_amd import api
    cloud = api.Cloud(ctx, N)
    integral = np.full(10 * N, -7.0, np.float32); index = np.full(N, -7, np.int32); rowoff = np.full(b.rows * 2, -7, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    for lean in (3, -1):
        rc = ctx._L.pwn_hip_debug_front_end(ctx.h, C.addressof(p), (C.c_void_p * 1)(src.ctypes.data), 0.0, 1, b.rows, b.cols, D.SINGLE_PASS, lean,
                                            (C.c_void_p * 1)(cloud.h.value), vp(integral), vp(index), None, vp(rowoff))
        assert rc == 1, rc
        assert (integral == -7.0).all() and (index == -7).all() and (rowoff == -7).all()


@pytest.mark.parametrize("path", [D.LATENCY, D.SINGLE_PASS])
def test_hand_over_time_out_is_reported_as_in_a_convert_call(ctx, made, path):
    """pwn_hip_debug_withhold_carry withholds one hand-over word (strip 0 -> 1, band 1, chain 37; 4096 polls keep it short, as test_handover.py
    does for the convert calls): the hook returns PWN_HIP_ERR_LAUNCH with the convert call's message, twice (the flag is reset), does not repeat
    the launch, and with the word back the same context gives the oracle's bits again"""
    import ctypes as C
    from g2o_frontend_amd._lib import PwnHipError
    b, ref, p = made(17, 129, "float")
    frames = window(3 if path == D.LATENCY else 16, 2)
    n0 = C.c_int(-1); n1 = C.c_int(-1)
    ctx.check(ctx._L.pwn_hip_debug_convert_retries(ctx.h, C.byref(n0)))
    ctx.check(ctx._L.pwn_hip_debug_withhold_carry(ctx.h, 0, 1, 37, b.rows, 4096))
    try:
        for _ in range(2):
            with pytest.raises(PwnHipError) as e:
                D.run_gpu(ctx, p, b, frames, path, 0)
            assert e.value.code == 5 and "strip hand-over timed out" in str(e.value)
    finally:
        ctx.check(ctx._L.pwn_hip_debug_withhold_carry(ctx.h, -1, 0, 0, b.rows, 0))
    ctx.check(ctx._L.pwn_hip_debug_convert_retries(ctx.h, C.byref(n1)))
    assert n1.value == n0.value, "the hook repeated a launch"
    run_and_compare(ctx, b, ref, p, frames, path, 0)


# ------------------------------------------------------------------------------------------------ the public calls on the same frames
def _converter(conf_name):
    from g2o_frontend_amd import api
    conf = D.CONFIGS[conf_name]
    K = conf["K"]
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    proj.setMinDistance(conf["min_distance"]); proj.setMaxDistance(conf["max_distance"])
    stats = api.StatsCalculatorIntegralImage()
    stats.setWorldRadius(D.STATS["world_radius"]); stats.setMinImageRadius(D.STATS["min_image_radius"])
    stats.setMaxImageRadius(D.STATS["max_image_radius"]); stats.setMinPoints(D.STATS["min_points"])
    return api.DepthImageConverterIntegralImage(proj, stats, api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator())


def _same_cloud(o, g, stats):
    """test_gpu_parity._compare_clouds' rule per field (same bits; +0 / -0 are the same number), NaN in the same place counted as equal"""
    assert len(o["points"]) == len(g["points"])
    if len(o["points"]) == 0:                  # the all-invalid frame
        return
    for k in ("points", "normals", "curvature", "omega_p", "omega_n"):
        a, c = o[k].reshape(len(o[k]), -1), g[k].reshape(len(g[k]), -1)
        same = D.same_bits(a, c) | ((a == 0) & (c == 0))
        assert same.all(), f"{k}: {int((~same).any(1).sum())} of {len(a)} points differ"
    if stats:
        assert np.array_equal(o["npoints"], g["npoints"])
        assert D.same_bits(o["eigenvalues"], g["eigenvalues"]).all()
        ok = o["npoints"] > 0
        assert D.same_bits(o["stats"][ok], g["stats"][ok]).all()


@pytest.mark.parametrize("shape", [(17, 129), (129, 513)])
@pytest.mark.parametrize("kind", ["float", "raw"])
def test_convert_calls_agree_with_oracle_on_the_same_frames(ctx, made, oracle, shape, kind):
    """the noise and the pattern frames through converter.computeBatch in one launch of at least 16 frames (the single-pass kernel, lean) and through
    converter.compute frame by frame with keep_stats (the latency path, lean = 0), both against oracle.convert as test_gpu_fuzz compares"""
    from g2o_frontend_amd import api
    rows, cols = shape
    b, _, p = made(rows, cols, kind)
    frames = [i for i, k in enumerate(b.kinds) if k not in ("edges", "overflow", "nan")]
    assert len(frames) >= 16 and not b.undefined_mask()[frames].any()
    conv = _converter(b.conf_name)
    depth = [oracle.convert_16u_to_32f(b.frames[i], b.scale) if kind == "raw" else b.frames[i] for i in frames]
    want = [oracle.convert(p, d) for d in depth]
    clouds = [api.Cloud(ctx, rows * cols) for _ in frames]
    conv.computeBatch(clouds, [np.ascontiguousarray(b.frames[i]) for i in frames], raw_scale=b.scale if kind == "raw" else None)
    ran = {s: ctx.stage_ms(s)[1] for s in STAGES}
    assert ran["integral"] == 1 and ran["integral_rows"] == 0 and ran["stats"] == 1, ran
    normals = 0
    for (oc, _, _), g in zip(want, clouds):
        o = oc.arrays()
        _same_cloud(o, g.arrays(), stats=False)
        normals += int((np.abs(o["normals"][:, :3]).sum(1) > 0).sum())
    assert normals > 1000, "degenerate input: the stats pass produced no normals to compare"
    for (oc, oidx, oitv), d in zip(want, depth):
        cloud = api.Cloud(ctx, rows * cols)
        conv.compute(cloud, d, keep_stats=True)
        ran = {s: ctx.stage_ms(s)[1] for s in STAGES}
        assert ran["integral_rows"] == 1 and ran["integral"] == 0, ran
        assert np.array_equal(oidx, conv.indexImage()) and np.array_equal(oitv, conv.intervalImage())
        _same_cloud(oc.arrays(stats=True), cloud.arrays(stats=True), stats=True)
