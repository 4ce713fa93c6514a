"""The injected aligner clouds (tests/align_clouds.py) on the CPU: the oracle's projection gives the index images the generator intended, the
oracle and the numpy model agree on these clouds, and every family reaches the branch it claims -- counted from the oracle and the model
alone; the counts are conditions of the test.  Also measured here, from the reference side only: the distance between the oracle's fp32
Gauss-Newton step and the model's float64 step on these cases (docs/parity.md; tests/test_gpu_align_clouds.py derives its pose bar from
ORACLE_STEP_DISTANCE below)."""
import numpy as np
import pytest

import align_clouds as A
import numpy_reference_model as M

f32 = np.float32
# worst |oracle fp32 step - float64 step| over the case set, as test_step_distance_of_the_oracle measures it (it asserts the measured value stays
# below this figure, so the GPU test's bar max(5e-6, 4 x this) cannot drift unnoticed)
ORACLE_STEP_DISTANCE = 1e-6      # measured: 9.2e-7 (mixed64x32, robust kernel off)
# the same on the cases run in the converter's form (class matrices by the curvature rule in place of the injected Omega_n), as
# tests/test_flat_clouds_cpu.py::test_step_distance_on_converter_form_cases measures and asserts it; tests/test_gpu_converter_form.py's pose bar
CONVERTER_FORM_STEP_DISTANCE = 1e-6      # measured: 7.2e-7 (mixed64x32, cls_thr 0.01, rotated table, robust kernel off)


def _check_case(O, case):
    """projection, finder and linearizer of one case: oracle against generator and model.  Returns (terms, accepted mask, corr, local errors)."""
    p = case.params
    oref, ocur, ra, ca = A.oracle_clouds(O, case)
    ri, _ = O.project(case.K, case.guess, p["min_distance"], p["max_distance"], case.rows, case.cols, ra["points"])
    ci, _ = O.project(case.K, np.eye(4), p["min_distance"], p["max_distance"], case.rows, case.cols, ca["points"])
    assert np.array_equal(ri, case.ref_index), (case.name, int((ri != case.ref_index).sum()))
    assert np.array_equal(ci, case.cur_index), (case.name, int((ci != case.cur_index).sum()))
    mi, _ = M.project(ra["points"][:, :3], M.projector_matrices(case.K, case.guess)[0], p["min_distance"], p["max_distance"], case.rows, case.cols)
    assert np.array_equal(mi, ri), case.name
    Tinv = O.iso_inverse(case.guess)
    ap = A.oracle_params(O, case)
    ocorr, oK = O.correspondences(ap, oref, ocur, ri, ci, Tinv)
    args = (p["inlier_normal_angular_threshold"], p["inlier_distance_threshold"], p["flat_curvature_threshold"], p["inlier_curvature_ratio_threshold"])
    mcorr, mK = M.correspondences(ra, ca, ri, ci, Tinv, *args)
    assert oK == mK == int(case.candidates().sum()) and np.array_equal(ocorr, mcorr), case.name
    t = M.correspondence_terms(ra, ca, ri, ci, Tinv, p["flat_curvature_threshold"])
    acc = np.zeros(len(t["ri"]), bool)
    pos = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(t["ri"], t["ci"]))}
    acc[[pos[(int(a), int(b))] for a, b in ocorr]] = True
    for robust in (1, 0):
        apr = A.oracle_params(O, case, robust_kernel=robust)
        ol = O.linearize(apr, oref, ocur, ocorr, Tinv)
        H, b, chi2, inl, Habs, babs = M.linearize(ra, ca, ocorr, Tinv, p["inlier_max_chi2"], bool(robust), abs_sums=True)
        le = M.local_error_f32(ra, ca, ocorr, Tinv)
        # inliers are decided by fp32 local errors: the float64 model may differ on terms within rounding of the threshold only
        assert ol["inliers"] == (len(le) if robust else int((~(le > f32(p["inlier_max_chi2"]))).sum())), case.name
        if ol["inliers"] == inl:
            # as tests/test_oracle_vs_numpy_model.py: counters equal, chi2 within 1e-5 of the model's float64 sums (the step itself: see
            # test_step_distance_of_the_oracle)
            # plus what the reference's fp32 remap of the point and the normal moves the errors by (see _fp32_chi2_slack)
            slack = _fp32_chi2_slack(ra, ca, ocorr, Tinv)
            assert abs(ol["chi2_fp64"] - chi2) <= 1e-5 * chi2 + slack, (case.name, robust, ol["chi2_fp64"], chi2, slack)
    return t, acc, ocorr, M.local_error_f32(ra, ca, ocorr, Tinv), (oref, ocur, ra, ca)


def _fp32_chi2_slack(ref, cur, corr, Tinv):
    """How far the oracle's chi2 (fp32 terms, as the reference computes them) may lie from the model's float64 one beyond the 1e-5 of
    tests/test_oracle_vs_numpy_model.py.  Isometry3f * Vector4f rounds three times per component, each time by at most 2^-24 of the partial sum:
    dp_i <= 3 * 2^-24 * sum_k |T_ik| |p_k|.  On converter clouds the point error is centimetres and this is hidden in the 1e-5; here errors go down
    to a millimetre at 4.4 m.  d(e' Omega e) <= 2 |e|' |Omega| de, and the fp32 evaluation of the form itself adds 8 roundings of its magnitude."""
    if not len(corr):
        return 0.0
    u = 2.0 ** -24
    T = np.abs(np.asarray(Tinv, np.float64))
    ri, ci = corr[:, 0], corr[:, 1]
    dp = 3 * u * (np.abs(ref["points"][ri, :3].astype(np.float64)) @ T[:3, :3].T + T[:3, 3]) + u * np.abs(cur["points"][ci, :3])
    dn = 3 * u * (np.abs(ref["normals"][ri, :3].astype(np.float64)) @ T[:3, :3].T) + u * np.abs(cur["normals"][ci, :3])
    Tf = np.asarray(Tinv, np.float64)
    pe = np.abs(ref["points"][ri, :3].astype(np.float64) @ Tf[:3, :3].T + Tf[:3, 3] - cur["points"][ci, :3])
    ne = np.abs(ref["normals"][ri, :3].astype(np.float64) @ Tf[:3, :3].T - cur["normals"][ci, :3])
    oP = np.abs(cur["omega_p"][ci].reshape(-1, 4, 4).transpose(0, 2, 1)[:, :3, :3].astype(np.float64))
    oN = np.abs(cur["omega_n"][ci].reshape(-1, 4, 4).transpose(0, 2, 1)[:, :3, :3].astype(np.float64))
    q = lambda a, o, b: np.einsum("ni,nij,nj->n", a, o, b)
    return float((2 * q(pe, oP, dp) + 2 * q(ne, oN, dn) + 8 * u * (q(pe, oP, pe) + q(ne, oN, ne))).sum())


def _count(d, k, n=1):
    d[k] = d.get(k, 0) + int(n)


def test_families_reach_their_branches(oracle):
    O = oracle
    cand, cover = {}, {}
    for case in A.cpu_case_set():
        t, acc, corr, le, _ = _check_case(O, case)
        p = case.params
        fam = case.family[t["pixel"]]; sub = case.sub[t["pixel"]]
        assert (fam != "").all(), "a candidate without a family"
        for f in A.FAMILIES:
            _count(cand, f, (fam == f).sum())
        # intended outcomes
        exp = case.expect[t["pixel"]]
        assert (acc[exp == 1]).all() and not acc[exp == 0].any(), case.name
        ident = case.guess_name == "identity"
        thr = f32(p["inlier_normal_angular_threshold"]); sq = f32(p["inlier_distance_threshold"]) * f32(p["inlier_distance_threshold"])
        mx = f32(p["inlier_curvature_ratio_threshold"]); mn = f32(1.0) / mx
        zn = fam == "zero_normal"
        sqn = np.minimum(t["sq_cn"], t["sq_rn"]); tiny = np.finfo(f32).tiny
        _count(cover, "zero_normal exact zero", (zn & (sqn == 0) & np.char.startswith(sub.astype(str), "zero")).sum())
        _count(cover, "zero_normal under: squares underflow to 0, rejected", (zn & (sqn == 0) & np.char.startswith(sub.astype(str), "under") & ~acc).sum())
        d23 = zn & (sqn > 0) & (sqn < tiny) & np.char.startswith(sub.astype(str), "denorm")
        _count(cover, "zero_normal denormal squared norm", d23.sum())
        if p["inlier_normal_angular_threshold"] <= 0:
            assert acc[d23].all(), "a normal with a denormal squared norm must pass"
            _count(cover, "zero_normal denormal accepted", (d23 & acc).sum())
        assert not (zn & (sqn == 0) & acc).any()
        live = (t["sq_cn"] != 0) & (t["sq_rn"] != 0)
        na = (fam == "normal_angle") & live
        if ident:
            _count(cover, "normal_angle at equality", (na & (t["dot"] == thr)).sum())
            for k in (1, 2, 3, 4):
                _count(cover, "normal_angle 1..4 ulps below", (na & (A.ulps(t["dot"], thr) == -k)).sum()); _count(cover, "normal_angle 1..4 ulps above", (na & (A.ulps(t["dot"], thr) == k)).sum())
            assert acc[na & (t["dot"] == thr)].all()             # '<': equality passes
        _count(cover, "normal_angle within 1e-6", (na & (np.abs(t["dot"].astype(np.float64) - float(thr)) < 1e-6)).sum())
        di = (fam == "distance") & live
        if ident:
            _count(cover, "distance at equality", (di & (t["sqdist"] == sq)).sum())
            for k in (1, 2, 3, 4):
                _count(cover, "distance 1..4 ulps below", (di & (A.ulps(t["sqdist"], sq) == -k)).sum()); _count(cover, "distance 1..4 ulps above", (di & (A.ulps(t["sqdist"], sq) == k)).sum())
            assert acc[di & (t["sqdist"] == sq)].all()           # '>': equality passes
        _count(cover, "distance within 1e-6", (di & (np.abs(t["sqdist"].astype(np.float64) - float(sq)) < 1e-6)).sum())
        ra_ = fam == "ratio"
        est = (t["rc"] + f32(1e-5)) / (t["cc"] + f32(1e-5))
        band = ra_ & (((est >= mn * (f32(1) - f32(1e-5))) & (est <= mn * (f32(1) + f32(1e-5)))) | ((est >= mx * (f32(1) - f32(1e-5))) & (est <= mx * (f32(1) + f32(1e-5)))))
        _count(cover, "ratio in the estimate band", band.sum()); _count(cover, "ratio in the band, accepted", (band & acc).sum())
        _count(cover, "ratio in the band, rejected", (band & ~acc).sum())
        _count(cover, "ratio at a bound", (ra_ & ((t["ratio"] == mn) | (t["ratio"] == mx))).sum())
        _count(cover, "ratio 1..3 ulps off a bound", (ra_ & ((np.abs(A.ulps(t["ratio"], mn)) <= 3) | (np.abs(A.ulps(t["ratio"], mx)) <= 3)) & (t["ratio"] != mn) & (t["ratio"] != mx)).sum())
        _count(cover, "ratio outside the band beyond a bound", (ra_ & ~band & ~acc).sum())
        rcur = case.ref["curvature"][t["ri"]]; ccur = case.cur["curvature"][t["ci"]]; flat = f32(p["flat_curvature_threshold"])
        _count(cover, "ratio curvature exactly 0", (ra_ & ((rcur == 0) | (ccur == 0))).sum())
        _count(cover, "ratio curvature at flatThr", (ra_ & ((rcur == flat) | (ccur == flat))).sum())
        _count(cover, "ratio curvature an ulp off flatThr", (ra_ & ((np.abs(A.ulps(np.maximum(rcur, f32(1e-3)), flat)) == 1) | (np.abs(A.ulps(np.maximum(ccur, f32(1e-3)), flat)) == 1))).sum())
        _count(cover, "ratio both clamped", (ra_ & (rcur < flat) & (ccur < flat)).sum())
        # local errors of the accepted
        pixel_of = {(int(a), int(b)): int(px) for a, b, px in zip(t["ri"], t["ci"], t["pixel"])}
        cpix = np.array([pixel_of[(int(a), int(b))] for a, b in corr], np.int64)
        cf = case.family[cpix] if len(cpix) else np.zeros(0, object)
        mc = f32(p["inlier_max_chi2"]); ce = cf == "chi2_edge"
        if ident:
            _count(cover, "chi2_edge at equality", (ce & (le == mc)).sum())
            for k in (1, 2, 3, 4):
                _count(cover, "chi2_edge 1..4 ulps below", (ce & (A.ulps(np.maximum(le, f32(1)), mc) == -k)).sum()); _count(cover, "chi2_edge 1..4 ulps above", (ce & (A.ulps(np.maximum(le, f32(1)), mc) == k)).sum())
        _count(cover, "chi2_edge 1e3..1e8 above", (ce & (le > f32(1e3) * mc)).sum())
        om = cf == "omega_range"
        opn = np.abs(case.cur["omega_p"][corr[:, 1]]).max(1) if len(corr) else np.zeros(0)
        _count(cover, "omega_range zero Omega_p", (om & (opn == 0)).sum()); _count(cover, "omega_range |Omega_p| > 1e6", (om & (opn > 1e6)).sum())
        _count(cover, "index_edges accepted", (cf == "index_edges").sum())
        for kind in ("multi2", "multi3", "tie2", "tie3", "depth_at", "pixel0", "pixelN1", "column8", "tile_last"):
            _count(cover, f"index_edges {kind}", ((fam == "index_edges") & (sub == kind)).sum())
        ie = case.family == "index_edges"
        _count(cover, "index_edges one side / out of range (no candidate)", (ie & ~case.candidates()).sum())
        if case.name.startswith("cancel/"):
            H, b, _, _, Habs, babs = M.linearize(case.ref, case.cur, corr, O.iso_inverse(case.guess), p["inlier_max_chi2"], True, abs_sums=True)
            rb = np.abs(b[:3]) / babs[:3]; rh = np.abs(H[:3, 3:]) / np.maximum(Habs[:3, 3:], 1e-300)
            assert rb.min() <= 1e-4 and rh.min() <= 1e-4, (case.name, rb, rh)
            _count(cover, "cancel cases with a b and an Htr residue <= 1e-4 of the magnitudes")
        if case.name.startswith("empty"):
            assert len(corr) == 0
            _count(cover, "empty " + ("no candidate" if len(t["ri"]) == 0 else "candidates, no correspondence"))
    print("candidates per family:", cand)
    for k in sorted(cover):
        print(f"  {k:70s} {cover[k]}")
    for f in A.FAMILIES:
        # `empty` holds candidates in its "rejected" kind only; class_edge is in no case of this set (tests/test_flat_clouds_cpu.py holds its floors)
        if f not in ("empty", "class_edge"):
            assert cand[f] >= 50, (f, cand[f])
    need = {"normal_angle at equality": 20, "distance at equality": 20, "chi2_edge at equality": 20, "ratio in the estimate band": 50,
            "ratio in the band, accepted": 10, "ratio in the band, rejected": 10, "zero_normal denormal accepted": 10,
            "zero_normal under: squares underflow to 0, rejected": 10, "zero_normal exact zero": 10, "zero_normal denormal squared norm": 10}
    for k in ("normal_angle", "distance", "chi2_edge"):
        need[f"{k} 1..4 ulps below"] = 20; need[f"{k} 1..4 ulps above"] = 20
    for k in ("ratio at a bound", "ratio 1..3 ulps off a bound", "ratio curvature exactly 0", "ratio curvature at flatThr", "ratio curvature an ulp off flatThr",
              "ratio both clamped", "chi2_edge 1e3..1e8 above", "omega_range zero Omega_p", "omega_range |Omega_p| > 1e6", "index_edges multi2", "index_edges multi3",
              "index_edges tie2", "index_edges tie3", "index_edges depth_at", "index_edges column8", "index_edges one side / out of range (no candidate)"):
        need[k] = 10
    for k in ("index_edges pixel0", "index_edges pixelN1", "index_edges tile_last", "empty no candidate", "empty candidates, no correspondence",
              "cancel cases with a b and an Htr residue <= 1e-4 of the magnitudes"):
        need[k] = 2
    for k, n in need.items():
        assert cover.get(k, 0) >= n, (k, cover.get(k, 0), n)


def test_large_sizes_sit_on_the_reduction_boundary():
    """reduce_partials takes 160 records per trip: 512x640 ends on the last record of the first trip, 513x640 puts one record into the second"""
    for (rows, cols), nt in zip(A.LARGE_SIZES, (150, 160, 161)):
        case = A.mixed_case(rows, cols)
        assert case.tiles == nt
        has = np.unique(np.nonzero(case.candidates())[0] // A.TILE)
        want = {0, 3, 7, nt - 1} | {k for k in range(156, 161) if k < nt}
        assert want <= set(has.tolist()), (rows, has)
        lone = np.nonzero(case.candidates())[0]; lone = lone[lone // A.TILE == 7]
        assert lone.tolist() == [8 * A.TILE - 1]
        assert int(case.candidates().sum()) <= 60000


def test_step_distance_of_the_oracle(oracle):
    """the oracle's fp32 step (H + 1001 I, LDL^T, v2t, t2v) against the model's float64 step, one iteration from the case's guess"""
    worst, where = 0.0, None
    for case in A.cpu_case_set():
        oref, ocur, ra, ca = A.oracle_clouds(oracle, case)
        for over in ({}, {"robust_kernel": 0}):
            d, _ = A.step_distance(oracle, M, case, ra, ca, oref, ocur, **over)
            print(f"  {case.name:28s} robust {over.get('robust_kernel', 1)}: {d:.3e}")
            if d > worst:
                worst, where = d, (case.name, over)
    print(f"worst oracle-to-float64 step distance {worst:.3e} at {where}")
    assert worst <= ORACLE_STEP_DISTANCE
