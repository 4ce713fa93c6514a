"""The cloud-level fusion on the GPU: pwn_hip_merge_clouds against the numpy model of Merger2::merge (tests/merge_clouds.py), every array of
the total cloud and the weights bit for bit, on injected and natural lists; one list against the same clouds in single and split calls; host
and device weights; refusals; PwnMerger.mergeNodeList end to end; the C++ mirror's check tool; Cloud.add through the shared device function."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_clouds as MC      # noqa: E402
from conftest import case_params      # noqa: E402
from test_omega_sym6 import LOWER, UPPER      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID, CAPACITY = 1, 6


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


def Kc(K):
    return np.array([K[0], 0, 0, 0, K[1], 0, K[2], K[3], 1], F)


def Km(K):
    return np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], F)


def colmajor(T):
    return np.ascontiguousarray(np.asarray(T, F).T).reshape(-1)


def upload(ctx, a, capacity=None):
    from g2o_frontend_amd import api
    n = len(a["points"])
    c = api.Cloud(ctx, max(1, n if capacity is None else capacity))
    if n:
        c.upload(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])
    return c


def merge_call(ctx, proj, clouds, transforms, total, weights, counts=True):
    """pwn_hip_merge_clouds -> (status, appended[n], fused[n]); total / weights are written in place"""
    K, offset, mn, mx, rows, cols = proj
    n = len(clouds)
    handles = (C.c_void_p * max(1, n))(*[c.h for c in clouds])
    tr = np.ascontiguousarray(np.stack([colmajor(T) for T in transforms]), F) if n else np.zeros((1, 16), F)
    app = (C.c_int * max(1, n))(*([-7] * max(1, n))); fus = (C.c_int * max(1, n))(*([-7] * max(1, n)))
    rc = ctx._L.pwn_hip_merge_clouds(ctx.h, ptr(Kc(K)), ptr(colmajor(offset)), n, handles, ptr(tr), mn, mx, rows, cols, total.h, ptr(weights),
                                     app if counts else None, fus if counts else None)
    return rc, np.array(list(app)[:n], np.int32), np.array(list(fus)[:n], np.int32)


def downloaded(total, weights, stats=True):
    """the total cloud and its weights as the model keeps them (stats=False: a cloud no merge has given Stats yet)"""
    n = total.size()
    t = total.arrays(stats=stats)
    w = weights if isinstance(weights, np.ndarray) else weights.numpy()
    t["weights"] = np.array(w[:n], F)
    t["gauss"] = total.gaussians() if total.numGaussians() else None
    assert t["gauss"] is None or len(t["gauss"]["flags"]) == n
    return t


def assert_total(got, want, what, sym6=False, exact_upper=True):
    assert len(got["points"]) == len(want["points"]), what
    for k in MC.CLOUD_KEYS + ("weights",):
        if sym6 and k == "omega_p":
            continue
        assert np.array_equal(MC.bits(got[k]), MC.bits(want[k])), (what, k, int((MC.bits(got[k]) != MC.bits(want[k])).sum()))
    if sym6:      # as tests/test_omega_sym6.py compares: the stored upper triangle, mirrored by the download
        a, b = want["omega_p"], got["omega_p"]
        for lo, up in LOWER:
            assert np.array_equal(MC.bits(b[:, lo]), MC.bits(b[:, up])), what
        if exact_upper:                   # sources whose matrices are exactly symmetric: the upper triangle carries the model's bits
            assert np.array_equal(MC.bits(a[:, UPPER]), MC.bits(b[:, UPPER])), what
        else:                             # converter-made sources: the mirrored lower triangle is another rounding of the same products
            fin = np.isfinite(a).all(1)
            s = np.abs(a[fin]).max(1, keepdims=True)
            assert (np.abs(a[fin] - b[fin]) <= 2e-6 * s).all(), what
            assert np.array_equal(np.isfinite(a).all(1), np.isfinite(b).all(1)), what
    assert (got["gauss"] is None) == (want["gauss"] is None), what
    if want["gauss"] is not None:
        og, gg = want["gauss"], got["gauss"]
        assert np.array_equal(og["flags"], gg["flags"]), what
        m, i = (og["flags"] & 1) != 0, (og["flags"] & 2) != 0
        for k, sel in (("mean", m), ("cov", m), ("info", i), ("info_vec", i)):
            assert np.array_equal(MC.bits(og[k][sel]), MC.bits(gg[k][sel])), (what, k)


def raw_state(total, weights, stats=True):
    """every downloaded byte, for comparisons between GPU runs"""
    t = downloaded(total, weights, stats)
    out = [t[k].tobytes() for k in MC.CLOUD_KEYS + ("weights",) if k in t]
    if t["gauss"] is not None:
        out += [t["gauss"][k].tobytes() for k in MC.GAUSS_KEYS]
    return out


# ------------------------------------------------------------------------------------------------------------ injected lists
def injected_on_gpu(ctx, c):
    """the case's total (with room for the whole list), its weights and its clouds on the device; identical sources share one cloud"""
    cap = len(c["total"]["points"]) + sum(len(s["points"]) for s in c["sources"])
    total = upload(ctx, c["total"], capacity=cap)
    w = np.full(max(1, cap), -5, F); w[:len(c["weights"])] = c["weights"]
    made = {}
    clouds = []
    for s in c["sources"]:
        if id(s) not in made:
            made[id(s)] = upload(ctx, s)
        clouds.append(made[id(s)])
    return total, w, clouds


def run_injected(ctx, rows, cols, sym6=False):
    for n, ranges, moved in MC.injected_variants(rows, cols):
        c = MC.injected_case(rows, cols, n, ranges, moved)
        want, wa, wf, _, _ = MC.merge_list(MC.total_from_arrays(c["total"], c["weights"]), MC.oracle_clouds(c), c["transforms"], c["proj"])
        what = (rows, cols, n, ranges, moved)
        total, w, clouds = injected_on_gpu(ctx, c)                            # pageable host weights
        rc, app, fus = merge_call(ctx, c["proj"], clouds, c["transforms"], total, w)
        assert rc == 0, what
        assert np.array_equal(app, wa) and np.array_equal(fus, wf), (what, app, wa, fus, wf)
        assert total.size() == len(want["points"]), what
        assert_total(downloaded(total, w), want, what, sym6=sym6)
        assert (w[total.size():] == -5).all(), what                           # nothing written past the points
        total2, w2, _ = injected_on_gpu(ctx, c)                               # device weights, no counters
        dw = ctx.upload(w2)
        rc, _, _ = merge_call(ctx, c["proj"], clouds, c["transforms"], total2, dw, counts=False)
        assert rc == 0, what
        assert raw_state(total2, dw) == raw_state(total, w), what
        assert (dw.numpy()[total2.size():] == -5).all(), what


@pytest.mark.parametrize("rows,cols", MC.SHAPES)
def test_injected_lists_bit_exact(ctx, oracle, rows, cols):
    run_injected(ctx, rows, cols)


def test_injected_lists_bit_exact_sym6(ctx6, oracle):
    run_injected(ctx6, 17, 129, sym6=True)


# ------------------------------------------------------------------------------------------------------------- natural lists
def converter_for(ctx, case):
    from g2o_frontend_amd import api
    conf, K = case["conf"], case["K"]
    proj = api.PinholePointProjector()
    proj.setCameraMatrix(Km(K)); proj.setMinDistance(conf["min_distance"]); proj.setMaxDistance(conf["max_distance"])
    proj.setImageSize(case["rows"], case["cols"])
    stats = api.StatsCalculatorIntegralImage()
    stats.setWorldRadius(conf["world_radius"]); stats.setMinImageRadius(conf["min_image_radius"]); stats.setMaxImageRadius(conf["max_image_radius"])
    stats.setMinPoints(conf["min_points"]); stats.setCurvatureThreshold(conf["stats_curvature_threshold"])
    pinfo, ninfo = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
    pinfo.setCurvatureThreshold(conf["point_info_curvature_threshold"]); ninfo.setCurvatureThreshold(conf["normal_info_curvature_threshold"])
    return api.DepthImageConverterIntegralImage(proj, stats, pinfo, ninfo)


def natural_on_gpu(ctx, case, n):
    """the first n frames converted on the device with Stats and Gaussians (bit for bit the oracle's clouds: tests/test_scene.py)"""
    from g2o_frontend_amd import api
    converter = converter_for(ctx, case)
    clouds = []
    for f in case["frames"][:n]:
        c = api.Cloud(ctx, case["rows"] * case["cols"])
        converter.compute(c, f, sensorOffset=case["offset"], keep_stats=True, gaussians=True)
        clouds.append(c)
    return clouds


def natural(rows, cols, with_offset=False):
    return MC.natural_case(rows, cols, MC.K_SMALL if rows == 60 else case_params("small")[2], with_offset=with_offset)


def fresh_total(ctx, clouds):
    from g2o_frontend_amd import api
    cap = sum(c.size() for c in clouds)
    return api.Cloud(ctx, max(1, cap)), np.full(max(1, cap), -5, F)


@pytest.mark.parametrize("rows,cols,with_offset", [(60, 80, False), (60, 80, True), (120, 160, False)])
def test_natural_lists_bit_exact(ctx, oracle, rows, cols, with_offset):
    case = natural(rows, cols, with_offset)
    clouds = natural_on_gpu(ctx, case, 9)
    for n in (1, 2, 3, 9):
        want, wa, wf, _, _ = MC.merge_list(MC.empty_total(gauss=True), case["clouds"][:n], case["transforms"][:n], case["proj"], gauss=True)
        total, w = fresh_total(ctx, clouds[:n])
        rc, app, fus = merge_call(ctx, case["proj"], clouds[:n], case["transforms"][:n], total, w)
        assert rc == 0
        assert np.array_equal(app, wa) and np.array_equal(fus, wf), (n, app, wa, fus, wf)
        assert_total(downloaded(total, w), want, (rows, cols, with_offset, n))
    if with_offset:
        return
    # one list == the same clouds in n calls of one cloud each == a list split 3 + 6, byte for byte (device weights for the split)
    one = raw_state(total, w)
    t1, w1 = fresh_total(ctx, clouds)
    for c, T in zip(clouds, case["transforms"]):
        assert merge_call(ctx, case["proj"], [c], [T], t1, w1)[0] == 0
    assert raw_state(t1, w1) == one
    t2, w2 = fresh_total(ctx, clouds)
    dw = ctx.upload(w2)
    assert merge_call(ctx, case["proj"], clouds[:3], case["transforms"][:3], t2, dw)[0] == 0
    assert merge_call(ctx, case["proj"], clouds[3:], case["transforms"][3:], t2, dw)[0] == 0
    assert raw_state(t2, dw) == one
    # sources without Stats and Gaussians (uploaded): the default Stats() under T, no Gaussians in the total
    bare = [MC.stripped(c) for c in case["clouds"][:3]]
    want = MC.merge_list(MC.empty_total(), bare, case["transforms"][:3], case["proj"])[0]
    up = [upload(ctx, c.arrays()) for c in bare]
    t3, w3 = fresh_total(ctx, up)
    assert merge_call(ctx, case["proj"], up, case["transforms"][:3], t3, w3)[0] == 0
    assert_total(downloaded(t3, w3), want, "bare")


def test_natural_list_sym6(ctx6, oracle):
    case = natural(60, 80)
    clouds = natural_on_gpu(ctx6, case, 3)
    want, wa, wf, _, _ = MC.merge_list(MC.empty_total(gauss=True), case["clouds"][:3], case["transforms"][:3], case["proj"], gauss=True)
    total, w = fresh_total(ctx6, clouds)
    rc, app, fus = merge_call(ctx6, case["proj"], clouds, case["transforms"][:3], total, w)
    assert rc == 0 and np.array_equal(app, wa) and np.array_equal(fus, wf)
    assert_total(downloaded(total, w), want, "sym6", sym6=True, exact_upper=False)


def test_vga_list_of_three(oracle):
    from g2o_frontend_amd import api, synth
    rows, cols = 480, 640
    case = MC.natural_case(rows, cols, synth.K_VGA, n=3)
    vga = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=3, omega_storage="exact9")
    try:
        clouds = natural_on_gpu(vga, case, 3)
        want, wa, wf, _, _ = MC.merge_list(MC.empty_total(gauss=True), case["clouds"], case["transforms"], case["proj"], gauss=True)
        total, w = fresh_total(vga, clouds)
        rc, app, fus = merge_call(vga, case["proj"], clouds, case["transforms"], total, w)
        assert rc == 0 and np.array_equal(app, wa) and np.array_equal(fus, wf)
        assert_total(downloaded(total, w), want, "vga")
        del clouds, total
    finally:
        vga.close()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_total_and_the_weights_untouched(ctx, ctx6, oracle):
    from g2o_frontend_amd import api
    rows, cols = 17, 129
    c = MC.injected_case(rows, cols, 2)
    K, offset, mn, mx, _, _ = c["proj"]
    L = ctx._L
    total, w, clouds = injected_on_gpu(ctx, c)
    dw = ctx.upload(w)
    before = raw_state(total, w, stats=False)                # uploaded: no Stats until a merge gives it the defaults
    other = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=1)
    foreign = api.Cloud(other, 16)
    six = upload(ctx6, c["sources"][0])                      # the other omega storage (and the other context)
    ctx._L.pwn_hip_ctx_set_omega_storage(ctx.h, 1)
    mixed = upload(ctx, c["sources"][0])                     # this context, the other omega storage
    ctx._L.pwn_hip_ctx_set_omega_storage(ctx.h, 0)
    assert mixed.omega_storage() == "sym6" and total.omega_storage() == "exact9"
    small = upload(ctx, c["total"])                          # a total with no room for the list
    ws = np.full(max(1, small.capacity), -5, F); ws[:len(c["weights"])] = c["weights"]
    small_before = raw_state(small, ws, stats=False)
    app = (C.c_int * 2)(-3, -3); fus = (C.c_int * 2)(-3, -3)
    tr = np.ascontiguousarray(np.stack([colmajor(MC.EYE)] * 2))
    h = lambda *cl: (C.c_void_p * 2)(*[x.h if x is not None else None for x in cl])      # noqa: E731
    ok = h(clouds[0], clouds[1])
    for wt in (w, dw):
        def args(ctxh=ctx.h, K_=ptr(Kc(K)), off=ptr(colmajor(offset)), n=2, cl=ok, t=ptr(tr), mn_=mn, mx_=mx, r=rows, co=cols, tot=total.h, wp=ptr(wt)):
            return (ctxh, K_, off, n, cl, t, mn_, mx_, r, co, tot, wp, app, fus)
        refused = [
            (INVALID, args(ctxh=None)), (INVALID, args(K_=None)), (INVALID, args(off=None)), (INVALID, args(cl=None)), (INVALID, args(t=None)),
            (INVALID, args(tot=None)), (INVALID, args(wp=None)), (INVALID, args(n=-1)),
            (INVALID, args(cl=h(clouds[0], None))),
            (INVALID, args(cl=h(clouds[0], foreign))), (INVALID, args(cl=h(clouds[0], six))),
            (INVALID, args(cl=h(clouds[0], total))),
            (INVALID, args(cl=h(clouds[0], mixed))),
            (CAPACITY, args(r=121, co=161)), (CAPACITY, args(r=1, co=19200)), (INVALID, args(r=0)),
            (INVALID, args(mn_=-0.01)),
        ]
        for want, a in refused:
            assert L.pwn_hip_merge_clouds(*a) == want, a
        assert L.pwn_hip_last_error_string(ctx.h)
        assert L.pwn_hip_merge_clouds(*args(n=0, cl=None, t=None)) == 0          # n == 0 writes nothing
    # the too-small total: refused on the upper bound before any work
    assert L.pwn_hip_merge_clouds(ctx.h, ptr(Kc(K)), ptr(colmajor(offset)), 2, ok, ptr(tr), mn, mx, rows, cols, small.h, ptr(ws), app, fus) == CAPACITY
    assert list(app) == [-3, -3] and list(fus) == [-3, -3]
    assert raw_state(total, w, stats=False) == before and raw_state(total, dw, stats=False) == before and total.size() == len(c["total"]["points"])
    with pytest.raises(api.PwnHipError):
        total.arrays(stats=True)                             # a refused call has not even given the total its Stats
    assert np.array_equal(dw.numpy().view(np.uint32), w.view(np.uint32))
    assert raw_state(small, ws, stats=False) == small_before
    # and the call still works afterwards
    rc, a2, f2 = merge_call(ctx, c["proj"], clouds, c["transforms"], total, w)
    want, wa, wf, _, _ = MC.merge_list(MC.total_from_arrays(c["total"], c["weights"]), MC.oracle_clouds(c), c["transforms"], c["proj"])
    assert rc == 0 and np.array_equal(a2, wa) and np.array_equal(f2, wf)
    assert_total(downloaded(total, w), want, "after the refusals")
    del foreign, six
    other.close()


# ------------------------------------------------------------------------------------------------- PwnMerger.mergeNodeList
NODE_SEED = 3


def node_list_input():
    """nine key frames of the seeded room at 120 x 160 and a tenth frame a small known motion away from the first"""
    from g2o_frontend_amd import synth
    from oracle import oracle as O
    case = natural(120, 160)
    motion = synth.pair_pose(NODE_SEED)
    tenth = O.convert_16u_to_32f(synth.render_depth_mm(NODE_SEED, case["poses"][0] @ motion, 120, 160, case["K"], hole_stream=9))
    return case, motion, tenth


def merger_objects(ctx, case):
    """the object graph at 120 x 160: the converter's projector is the merger's, matcher at scale 1"""
    from g2o_frontend_amd import api
    from test_gpu_parity import gpu_objects
    proj, converter, aligner = gpu_objects(ctx, "small")
    matcher = api.PwnMatcherBase(aligner, converter)
    matcher.setScale(1)
    return proj, converter, aligner, matcher


def test_merge_node_list_end_to_end(ctx, oracle):
    from g2o_frontend_amd import api
    case, motion, tenth = node_list_input()
    rows, cols, K = case["rows"], case["cols"], case["K"]
    eye = np.eye(4, dtype=F)
    proj, converter, aligner, matcher = merger_objects(ctx, case)
    cache = api.CloudCache(matcher, capacity=16)
    nodes = [api.MapNode(k, case["poses"][k]) for k in range(9)]
    for k in range(9):
        cache.addFrame(k, case["frames"][k], Km(K), eye)
    merger = api.Merger2(ctx, converter, matcher)
    pm = api.PwnMerger(merger, cache)
    fused = pm.mergeNodeList(nodes[0], nodes)
    assert cache.get(0) is fused and fused.capacity == fused.size() == merger.cloudTot().size()
    # the model on the oracle's conversions (no Stats kept, no Gaussians: what makeCloud gives), with the mirror's transforms
    trs = [api.PwnMerger.nodeTransform(nodes[0], o) for o in nodes]
    for T, Tm in zip(trs, case["transforms"]):
        assert np.allclose(T, Tm, rtol=0, atol=1e-6)
    bare = [MC.stripped(c) for c in case["clouds"]]
    want, wa, wf, _, _ = MC.merge_list(MC.empty_total(), bare, trs, case["proj"])
    assert merger.appended == wa.tolist() and merger.fused == wf.tolist()
    got = fused.arrays(stats=True)
    got["weights"] = merger.pesiTot(); got["gauss"] = None
    assert fused.numGaussians() == 0
    assert_total(got, want, "mergeNodeList")
    # a tenth frame against the fused cloud
    tc = matcher.makeCloud(Km(K), eye, tenth)[0]
    aligner.clearPriors()
    res = matcher.matchClouds(fused, tc, eye, eye, Km(K), rows, cols, np.eye(4))
    from test_gpu_parity import oracle_params
    cp, ap = oracle_params(oracle, "small", accumulate_fp64=1)
    oref = oracle.Cloud.from_arrays(want["points"], want["normals"], want["curvature"], want["omega_p"], want["omega_n"])
    ocur = oracle.convert(cp, tenth)[0]
    o = oracle.align(ap, oref, ocur)
    g = res["align"]
    it = o["iterations"][0]
    print("first iteration K / C / inliers:", int(g["K"][0]), int(g["C"][0]), int(g["iter_inliers"][0]), "oracle:", it["K"], it["C"], it["inliers"])
    assert (int(g["K"][0]), int(g["C"][0]), int(g["iter_inliers"][0])) == (it["K"], it["C"], it["inliers"])
    err = np.abs(res["transform"][:3, 3] - motion[:3, 3]).max()
    print("translation error against the rendered motion: %.2e" % err)
    assert err < 5e-3


# -------------------------------------------------------------------------------------------------------- the C++ check tool
def write_merge_file(path, case, sizes, n_total):
    """the input of tools/pwn_hip_merge_clouds_check: sizes, camera, range, the frames and poses, then what the Python mirror returned"""
    with open(path, "wb") as f:
        conf = case["conf"]
        f.write(struct.pack("<3i", case["rows"], case["cols"], len(case["frames"])))
        f.write(np.asarray(case["K"], np.float64).tobytes())
        f.write(struct.pack("<2d3i", conf["min_distance"], conf["max_distance"], conf["min_image_radius"], conf["max_image_radius"], conf["min_points"]))
        for fr, p in zip(case["frames"], case["poses"]):
            f.write(np.asarray(p, np.float64).tobytes())                    # row-major 4 x 4
            f.write(np.ascontiguousarray(fr, F).tobytes())
        f.write(struct.pack("<i", n_total))
        for name, a in sizes:
            b = np.ascontiguousarray(a).tobytes()
            f.write(struct.pack("<q", len(b))); f.write(b)


@pytest.mark.parametrize("rows,cols", [(60, 80), (120, 160)])
def test_cpp_mirror_gives_the_python_mirrors_cloud(oracle, tmp_path, rows, cols):
    from g2o_frontend_amd import api, build
    build.build_tools()
    case = natural(rows, cols)
    K = case["K"]
    eye = np.eye(4, dtype=F)
    own = api.Context(device=0, max_rows=rows, max_cols=cols, max_batch=9, omega_storage="exact9")
    try:
        converter = converter_for(own, case)
        aligner = api.Aligner(own); aligner.setProjector(converter.projector())
        matcher = api.PwnMatcherBase(aligner, converter); matcher.setScale(1)
        cache = api.CloudCache(matcher, capacity=16)
        nodes = [api.MapNode(k, case["poses"][k]) for k in range(9)]
        for k in range(9):
            cache.addFrame(k, case["frames"][k], Km(K), eye)
        merger = api.Merger2(own, converter, matcher)
        fused = api.PwnMerger(merger, cache).mergeNodeList(nodes[0], nodes)
        a = fused.arrays(stats=True)
        arrays = [(k, a[k]) for k in MC.CLOUD_KEYS] + [("weights", merger.pesiTot()), ("appended", np.array(merger.appended, np.int32)),
                                                       ("fused", np.array(merger.fused, np.int32))]
        path = str(tmp_path / "merge.bin")
        write_merge_file(path, case, arrays, fused.size())
        r = subprocess.run([os.path.join(ROOT, "tools", "pwn_hip_merge_clouds_check"), path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        del fused, cache, merger
    finally:
        own.close()


# ------------------------------------------------------------------------------------- Cloud::add through the shared function
def test_cloud_add_still_equals_the_oracle(ctx, oracle):
    """k_cloud_append and k_merge_clouds_append share one device function: Cloud.add against the oracle, non-identity T, Stats and Gaussians"""
    from g2o_frontend_amd import api
    case = natural(60, 80)
    g0, g1 = natural_on_gpu(ctx, case, 2)
    T = case["transforms"][5]
    oscene = oracle.Cloud(); gscene = api.Cloud(ctx, 2 * 60 * 80)
    for oc, gc, t in ((case["clouds"][0], g0, MC.EYE), (case["clouds"][1], g1, T)):
        oscene.add(oc, t); gscene.add(gc, t)
    oa, ga = oscene.arrays(stats=True), gscene.arrays(stats=True)
    assert len(oscene) == gscene.size()
    for k in oa:
        assert np.array_equal(MC.bits(oa[k]), MC.bits(ga[k])), k
    og, gg = oscene.gaussians(), gscene.gaussians()
    assert oscene.num_gaussians() == gscene.numGaussians() and np.array_equal(og["flags"], gg["flags"])
    m = (og["flags"] & 1) != 0
    assert np.array_equal(MC.bits(og["mean"][m]), MC.bits(gg["mean"][m])) and np.array_equal(MC.bits(og["cov"][m]), MC.bits(gg["cov"][m]))
