"""The aligner on injected clouds in the CONVERTER'S form (tests/flat_clouds.py: no Omega_n planes but a curvature threshold and two class
matrices, a stored index image under the library's own key; made through pwn_hip_cloud_import), in both Omega_p storages.  These are the
branches every production alignment takes: the class derived from the CURRENT point's curvature and the 27-float LDS table of the fused pass
(k_corr_linearize, k_corr_linearize_lat), load_omegas' class branch (k_linearize_list), the class expansion of the download and of
k_expand_omega_n, and the two projection shortcuts (the current cloud's own index image; the reference cloud's in iteration 0 of an identity
guess).  The oracle gets explicit Omega_n per point by the reference's rule (flat_clouds.omega_n_by_rule).

Checks are those of tests/test_gpu_align_clouds.py (_check_fused): the finder's four images bit for bit, (K, C, inliers) exact, chi2 within
CHI2_RTOL, H and b of the statistics pass and of Aligner.linearize per entry within (chain + 6) 2^-24 sum|term| + 2^-24 |o|, the pose after one
iteration within max(5e-6, 4 x CONVERTER_FORM_STEP_DISTANCE) (tests/test_flat_clouds_cpu.py measures that distance on these cases).

Launch forms: 1 single pairs (latency shape); 2 the 480 x 640 mixed case as 2 and 4 pairs (throughput shape); 3 the current index shortcut on
and off; 4 the reference index shortcut on and off; 5 a sub-batch that one uploaded cloud keeps from the shortcut; 6 the class rule off the
fused pass (download, Cloud::add).
"""
import ctypes as C

import numpy as np
import pytest

import align_clouds as A
import flat_clouds as FC
from test_align_clouds_cpu import CONVERTER_FORM_STEP_DISTANCE
from test_gpu_align_clouds import CHI2_RTOL, RESULT_FIELDS, STORAGES, _check_fused, _chi2_close, _compute_units

pytestmark = pytest.mark.gpu

STEP_BAR = max(5e-6, 4 * CONVERTER_FORM_STEP_DISTANCE)
_ctx = {}
_clouds = {}


@pytest.fixture(scope="module")
def rig():
    from g2o_frontend_amd import api

    def get(storage):
        if storage not in _ctx:
            _ctx[storage] = api.Context(device=0, max_rows=513, max_cols=683, max_batch=8, omega_storage=storage)
            _ctx[storage].set_profiling(True)      # the stage counters tell which projections a call launched
        return _ctx[storage]
    yield get
    _clouds.clear()
    for c in _ctx.values():
        c.check(c._L.pwn_hip_debug_set_index_shortcut(c.h, 1))
        c.close()
    _ctx.clear()


def maker(thr, tname, with_index=True):
    """cloud maker for _check_fused: both clouds in the converter's form, the oracle's with Omega_n by the rule.  The reference cloud stores
    its index image under the identity guess only (there case.ref_index IS its projection, tests/test_align_clouds_cpu.py).  Clouds are kept
    per (context, case, threshold, table): they are never written after their import."""
    def mk(ctx, case, storage, oracle):
        key = (id(ctx), case.name, thr, tname, with_index)
        if key not in _clouds:
            table = FC.TABLES[tname]
            g = (FC.converter_form(ctx, case, "ref", table, thr, with_index and case.guess_name == "identity"),
                 FC.converter_form(ctx, case, "cur", table, thr, with_index))
            ra, ca = FC.oracle_arrays(case, storage, table, thr)
            oc = lambda a: oracle.Cloud.from_arrays(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])
            _clouds[key] = (g, (oc(ra), oc(ca)), (ra, ca))
        return _clouds[key]
    return mk


def _fused(rig, oracle, case, storage, thr, tname, **over):
    return _check_fused(rig, oracle, case, storage, maker(thr, tname), STEP_BAR, CONVERTER_FORM_STEP_DISTANCE, **over)


def _report(tag, storage, rows):
    print(f"  {tag:16s} {storage}: {len(rows)} alignments, candidates {sum(r['K'] for r in rows)}, correspondences {sum(r['C'] for r in rows)}, "
          f"worst chi2 distance {max(r['chi2'] for r in rows):.2e}, worst H/b error {max(r['frac'] for r in rows):.3f} of its bar, worst step {max(r['step'] for r in rows):.2e}")


def _launches(ctx, stage):
    return ctx.stage_ms(stage)[1]


def _shortcut(ctx, on):
    ctx.check(ctx._L.pwn_hip_debug_set_index_shortcut(ctx.h, 1 if on else 0))


# ------------------------------------------------------------------------------------------------------------ 1. latency shape
OVERS = ({}, {"robust_kernel": 0}, {"inner_iterations": 2})


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("size", A.CLASS_EDGE_SIZES)
def test_class_edge_single_pairs(rig, oracle, storage, size):
    """three guesses x three thresholds x two tables; robust kernel off and a second inner iteration (SAME_T = false) under every guess"""
    rows = []
    for guess in A.GUESSES:
        for thr in A.CLASS_THRESHOLDS:
            case = A.class_edge_case(*size, guess, thr)
            for tname in ("shipped", "rotated"):
                for over in OVERS:
                    r = _fused(rig, oracle, case, storage, thr, tname, **over)
                    assert r["K"] == r["C"] == 900                      # every candidate a correspondence
                    rows.append(r)
    _report(f"class_edge {size}", storage, rows)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("fam", list(A.SMALL_SIZES))
def test_family_cases_single_pairs(rig, oracle, storage, fam):
    """every family of tests/align_clouds.py alone under the three guesses, with the rotated table and the shipped threshold"""
    rows = []
    for guess in A.GUESSES:
        case = A.family_case(fam, guess)
        for over in OVERS if fam in ("chi2_edge", "omega_range") else OVERS[:1]:
            rows.append(_fused(rig, oracle, case, storage, 0.02, "rotated", **over))
    _report(fam, storage, rows)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("size", A.CONVERTER_MIXED_SIZES)
def test_mixed_cases_single_pairs(rig, oracle, storage, size):
    """one tile, a second tile of one pixel, a partial tile, 150 tiles: three thresholds x two tables"""
    case = A.mixed_case(*size)
    rows = [_fused(rig, oracle, case, storage, thr, tname) for thr in A.CLASS_THRESHOLDS for tname in ("shipped", "rotated")]
    _report(f"mixed {size}", storage, rows)


# ------------------------------------------------------------------------------------------------------------ 2. throughput shape
def _batch_equals_singles(al, pairs, guesses, tag):
    """every pair of one alignBatch call equals its own call of one pair in every result field, bit for bit; returns the singles"""
    singles = [al.alignBatch([r], [c], [g], raw=True)[0].copy() for (r, c), g in zip(pairs, guesses)]
    res = al.alignBatch([r for r, _ in pairs], [c for _, c in pairs], guesses, raw=True)
    for k, one in enumerate(singles):
        for fld in RESULT_FIELDS:
            a, b = np.asarray(res[k][fld]), np.asarray(one[fld])
            assert a.tobytes() == b.tobytes(), (tag, k, fld, a, b)
    return singles


@pytest.mark.parametrize("storage", STORAGES)
def test_mixed_480x640_as_batches(rig, oracle, storage):
    """2 and 4 pairs of 150 tiles each: more workgroups than compute units (k_corr_linearize); one pair alone is the latency shape"""
    cus = _compute_units()
    ctx = rig(storage)
    base, moved = A.mixed_case(480, 640), A.mixed_case(480, 640, "moderate")
    assert base.tiles <= cus < 2 * base.tiles, (base.tiles, cus)
    variants = [(base, 0.02, "rotated"), (moved, 0.02, "rotated"), (base, 0.01, "shipped"), (base, 0.03, "rotated")]
    r0 = _fused(rig, oracle, base, storage, 0.02, "rotated")                     # pair 0 against the oracle: the clouds below are these clouds
    al = A.gpu_aligner(ctx, base)
    pairs = [maker(thr, t)(ctx, c, storage, oracle)[0] for c, thr, t in variants]
    guesses = [c.guess for c, _, _ in variants]
    for n in (2, 4):
        singles = _batch_equals_singles(al, pairs[:n], guesses[:n], f"{n} pairs")
        assert _launches(ctx, "project_cur") == 0                                  # every current cloud took its own index image
    al.setReferenceCloud(pairs[0][0]); al.setCurrentCloud(pairs[0][1]); al.setInitialGuess(base.guess)
    g = al.align()
    assert np.array_equal(g["T"].T.reshape(-1).view(np.uint32), singles[0]["T"].view(np.uint32))
    assert (int(g["K"][0]), int(g["C"][0])) == (r0["K"], r0["C"])


# ------------------------------------------------------------------------------------------------------------ 3., 4. the projection shortcuts
def _observe(ctx, al, stages):
    """one single alignment with statistics, then the score behind it, then the finder's four images: everything a caller can read, as bytes,
    and the launches the alignment call itself made of `stages`"""
    from g2o_frontend_amd import api
    g = al.align(statistics=True)
    n = {s: _launches(ctx, s) for s in stages}
    st = al._statistics
    m = api.MatchResult()
    ctx.check(ctx._L.pwn_hip_match_score(ctx.h, 50.0, C.byref(m)))                # before the images: off the cloud itself where the z-buffer is lazy
    al.align(images=True)
    f = al.correspondenceFinder()
    out = {k: np.ascontiguousarray(g[k]).tobytes() for k in ("T", "chi2", "iter_inliers", "C", "K")}
    out.update(error=g["error"], inliers=g["inliers"], iterations=g["iterations"])
    out.update({"stat_" + k: np.ascontiguousarray(st[k]).tobytes() for k in ("H", "b", "omega", "mean")}, stat_error=st["error"], stat_inliers=st["inliers"])
    out["score"] = (m.image_non_zeros, m.image_inliers, m.image_outliers, np.float32(m.image_reprojection_distance).tobytes())
    out.update({k: v.tobytes() for k, v in f._images.items()})
    return out, n, g


def _shortcut_cases():
    out = [(A.class_edge_case(*s, g, 0.02), 0.02, "rotated") for s in A.CLASS_EDGE_SIZES for g in A.GUESSES]
    out += [(A.mixed_case(*s), 0.02, "rotated") for s in A.CONVERTER_MIXED_SIZES]
    out += [(A.mixed_case(480, 640, "moderate"), 0.01, "shipped"), (A.family_case("index_edges"), 0.02, "rotated"), (A.family_case("zero_normal"), 0.02, "rotated")]
    return out


@pytest.mark.parametrize("storage", STORAGES)
def test_current_index_shortcut_is_the_projection(rig, oracle, storage):
    """the stored index image in place of projecting the current cloud: the same bits in everything a caller reads, one launch fewer"""
    ctx = rig(storage)
    try:
        for case, thr, tname in _shortcut_cases():
            (gref, gcur), _, _ = maker(thr, tname)(ctx, case, storage, oracle)
            al = A.gpu_aligner(ctx, case)
            al.setReferenceCloud(gref); al.setCurrentCloud(gcur)
            seen = {}
            for on in (1, 0):
                _shortcut(ctx, on)
                seen[on], n, _ = _observe(ctx, al, ("project_cur", "project_ref"))
                assert n == {"project_cur": 0 if on else 1, "project_ref": 1}, (case.name, on, n)
            assert seen[1].keys() == seen[0].keys()
            for k in seen[1]:
                assert seen[1][k] == seen[0][k], (case.name, k)
            assert np.array_equal(np.frombuffer(seen[1]["cur_index"], np.int32).reshape(case.rows, case.cols), case.cur_index)
    finally:
        _shortcut(ctx, 1)


@pytest.mark.parametrize("storage", STORAGES)
def test_reference_index_shortcut_is_the_projection(rig, oracle, storage):
    """identity guess, two outer iterations: the first takes the reference cloud's stored index image (no project_ref launch), the second
    projects; the same bits as with every projection executed; iteration 0 against the oracle's"""
    ctx = rig(storage)
    try:
        for case, thr, tname in _shortcut_cases():
            if case.guess_name != "identity":
                continue
            mk = maker(thr, tname)
            (gref, gcur), (oref, ocur), _ = mk(ctx, case, storage, oracle)
            al = A.gpu_aligner(ctx, case, outer_iterations=2)
            al.setReferenceCloud(gref); al.setCurrentCloud(gcur)
            seen = {}
            for on in (1, 0):
                _shortcut(ctx, on)
                seen[on], n, g = _observe(ctx, al, ("project_cur", "project_ref"))
                assert n == {"project_cur": 0 if on else 1, "project_ref": 1 if on else 2}, (case.name, on, n)
            for k in seen[1]:
                assert seen[1][k] == seen[0][k], (case.name, k)
            o = oracle.align(A.oracle_params(oracle, case, outer_iterations=2), oref, ocur)
            assert g["iterations"] == 2 == len(o["iterations"])
            i0 = o["iterations"][0]
            assert (int(g["K"][0]), int(g["C"][0]), int(g["iter_inliers"][0])) == (i0["K"], i0["C"], i0["inliers"]), case.name
            assert _chi2_close(float(g["chi2"][0]), i0["chi2_fp64"]), (case.name, float(g["chi2"][0]), i0["chi2_fp64"])
    finally:
        _shortcut(ctx, 1)


# ------------------------------------------------------------------------------------------------------------ 5. mixed sub-batch
@pytest.mark.parametrize("storage", STORAGES)
def test_one_uploaded_cloud_keeps_its_sub_batch_from_the_shortcut(rig, oracle, storage):
    """four pairs, the current cloud of pair 2 in the uploaded form (no index image): its sub-batch projects every current cloud, the other
    takes the stored images; in sub-batches of 4 and of 2 every pair equals its call alone"""
    ctx = rig(storage)
    cases = [A.class_edge_case(17, 65, g, 0.02) for g in ("identity", "small", "moderate")] + [A.class_edge_case(17, 65, "identity", 0.03)]
    pairs = [maker(c.cls_thr, "rotated")(ctx, c, storage, oracle)[0] for c in cases]
    up = A.gpu_clouds(ctx, cases[2])[1]                                              # the shipped table by the same rule, as explicit planes
    pairs[2] = (pairs[2][0], up)
    al = A.gpu_aligner(ctx, cases[0])
    try:
        for sub in (4, 2):
            ctx.set_subbatch(64, sub)
            _batch_equals_singles(al, pairs, [c.guess for c in cases], f"sub-batches of {sub}")
            assert _launches(ctx, "project_cur") == 1, sub                           # one sub-batch holds the uploaded cloud, in either split
            assert _launches(ctx, "corr_linearize") == 4 // sub
    finally:
        ctx.set_subbatch(64, 64)


# ------------------------------------------------------------------------------------------------------------ 6. the class rule off the fused pass
@pytest.mark.parametrize("storage", STORAGES)
def test_class_expansion_of_the_download_and_of_cloud_add(rig, oracle, storage):
    """Omega_n as the download expands the class table (cloud_fetch_records, host) and as Cloud::add expands it into a scene's planes
    (k_expand_omega_n) against the Omega_n handed to the oracle, bit for bit -- zero matrix where the fp32 squared norm of the normal is 0,
    which includes the zero_normal kinds whose components are near 1e-30 (their squares underflow)"""
    from g2o_frontend_amd import api
    ctx = rig(storage)
    cases = [(A.class_edge_case(*s, g, thr), thr, t) for s in A.CLASS_EDGE_SIZES for g in ("identity", "moderate") for thr in A.CLASS_THRESHOLDS
             for t in ("shipped", "rotated")]
    cases += [(A.family_case("zero_normal", g), 0.02, "rotated") for g in A.GUESSES] + [(A.mixed_case(17, 65), 0.01, "rotated")]
    seen = {0: 0, 1: 0, 2: 0, "underflow": 0}
    for case, thr, tname in cases:
        clouds, _, arrays = maker(thr, tname)(ctx, case, storage, oracle)
        for g, a in zip(clouds, arrays):
            want = a["omega_n"]
            cls = FC.classes_by_rule(a, thr)
            under = (cls == 0) & (a["normals"][:, :3] != 0).any(1)
            for k in (0, 1, 2):
                seen[k] += int((cls == k).sum())
            seen["underflow"] += int(under.sum())
            got = g.arrays()
            assert np.array_equal(got["curvature"].view(np.uint32), a["curvature"].view(np.uint32))
            bad = (got["omega_n"].view(np.uint32) != want.view(np.uint32)).any(1)
            assert not bad.any(), (case.name, "download", int(bad.sum()), int((bad & under).sum()))
            scene = api.Cloud(ctx, max(1, len(want)))
            scene.add(g)
            sgot = scene.arrays()["omega_n"]
            bad = (sgot.view(np.uint32) != want.view(np.uint32)).any(1)
            assert not bad.any(), (case.name, "Cloud::add", int(bad.sum()), int((bad & under).sum()))
    print(f"  {storage}: points per class {seen}")
    assert min(seen.values()) >= 100, seen
