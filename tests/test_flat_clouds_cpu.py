"""tests/flat_clouds.py and the class_edge family of tests/align_clouds.py on the CPU: the flat form read and written in numpy round-trips and has
the size the library says; the class_edge cases reach what they claim, counted from the oracle and the numpy model alone (floors are conditions
of the test); the inputs tell four wrong class rules apart by more than the H / b bar the GPU test applies; and the distance between the
oracle's fp32 step and the model's float64 step on the converter-form cases, from which tests/test_gpu_converter_form.py derives its pose bar."""
import numpy as np
import pytest

import align_clouds as A
import flat_clouds as FC
import numpy_reference_model as M
from test_align_clouds_cpu import CONVERTER_FORM_STEP_DISTANCE, _check_case

f32 = np.float32


def _random_flat(rng, n, sym, omn, shape):
    return dict(n=n, om_sym=sym, cls_thr=f32(rng.uniform(0.005, 0.05)), omN=rng.standard_normal((2, 9)).astype(f32), idx_K=rng.standard_normal(9).astype(f32),
                idx_min_d=f32(0.5), idx_max_d=f32(4.5), P3=rng.standard_normal((n, 3)).astype(f32), Nc=rng.standard_normal((n, 4)).astype(f32),
                Om=rng.standard_normal((FC.om_planes(sym), n, 3)).astype(f32), OmN=rng.standard_normal((3, n, 3)).astype(f32) if omn else None,
                index=rng.integers(-1, max(n, 1), shape).astype(np.int32) if shape else None)


@pytest.mark.parametrize("sym", (0, 1))
def test_flat_form_round_trips_and_has_the_library_size(sym):
    from g2o_frontend_amd import api
    rng = np.random.default_rng(11)
    storage = "sym6" if sym else "exact9"
    for n in (0, 1, 21, 22, 64, 1105, 2049):          # 12 n and 16 n on both sides of a multiple of 256 (12 * 64 = 768, 16 * 16 = 256)
        for omn in (False, True):
            for shape in (None, (1, 1), (3, 21), (17, 65)):
                x = _random_flat(rng, n, sym, omn, shape)
                buf = FC.write(x)
                assert FC.same(FC.parse(buf), x), (n, omn, shape)
                assert FC.same(FC.parse(FC.write(FC.parse(buf))), x)
                px = shape[0] * shape[1] if shape else 0
                assert buf.size == api.Cloud.flatBound(n, storage, px, omn), (n, storage, px, omn)
                if not omn:
                    assert buf.size == api._lib.lib().pwn_hip_cloud_export_bound(n, api.OMEGA_STORAGE[storage], px, 0)
    y = _random_flat(rng, 5, sym, True, (2, 3)); z = dict(y, P3=y["P3"].copy()); z["P3"][4, 2] = np.nextafter(z["P3"][4, 2], f32(9))
    assert not FC.same(y, z) and not FC.same(y, dict(y, OmN=None))


def test_tables():
    t = FC.TABLES["rotated"]
    assert t.dtype == f32 and t.shape == (2, 3, 3)
    for m, dg in zip(t, ((100, 50, 25), (1, 2, 3))):
        assert np.allclose(np.sort(np.linalg.eigvalsh(((m + m.T) / 2).astype(np.float64))), sorted(dg), rtol=1e-5)
        assert np.abs(m - m.T).max() <= 4 * np.finfo(f32).eps * np.abs(m).max()
        assert np.abs(m - np.diag(np.diag(m))).max() > 0.1 * max(dg) / 10              # a full matrix: off-diagonal entries far from 0
    assert (t != t.transpose(0, 2, 1)).any(), "mirror entries equal to the last bit: a transposed read would be the same table"
    assert np.array_equal(FC.TABLES["shipped"], np.stack([np.eye(3) * 100, np.eye(3)]).astype(f32))


def test_class_rule_on_the_zero_normal_kinds():
    """zero where the fp32 squared norm is 0: exact zeros AND components near 1e-30 (squares underflow); denormal squared norms keep their class"""
    case = A.family_case("zero_normal")
    for a in (case.ref, case.cur):
        cls = FC.classes_by_rule(a, 0.02)
        n = a["normals"][:, :3]
        exact0 = (n == 0).all(1); tiny = ~exact0 & (np.abs(n).max(1) < 1e-25); den = ~exact0 & ~tiny & (np.abs(n).max(1) < 1e-18)
        assert exact0.sum() >= 50 and tiny.sum() >= 50 and den.sum() >= 50
        assert (cls[exact0] == 0).all() and (cls[tiny] == 0).all() and (cls[den] > 0).all() and (cls[~exact0 & ~tiny] > 0).all()
        on = FC.omega_n_of_classes(cls, FC.TABLES["rotated"]).reshape(-1, 4, 4).transpose(0, 2, 1)
        assert not on[cls == 0].any() and np.array_equal(on[cls == 1][:, :3, :3], np.tile(FC.TABLES["rotated"][0], ((cls == 1).sum(), 1, 1)))


def _model_H(ra, ca, corr, Tinv, p, omega_n):
    c = dict(ca, omega_n=omega_n)
    H, b, _, _, Habs, babs = M.linearize(ra, c, corr, Tinv, p["inlier_max_chi2"], True, abs_sums=True)
    return H, b, Habs, babs


def test_class_edge_reaches_its_branches_and_tells_wrong_rules_apart(oracle):
    O = oracle
    rot = FC.TABLES["rotated"]
    total = {}
    for case in A.class_edge_cases():
        t, acc, corr, le, (oref, ocur, ra, ca) = _check_case(O, case)
        p = case.params; thr = f32(case.cls_thr)
        fam = case.family[t["pixel"]]; sub = case.sub[t["pixel"]]
        assert (fam == "class_edge").all() and len(fam) == 900
        assert acc.all(), (case.name, int((~acc).sum()))                     # every candidate is a correspondence
        # the ratio stays clear of the +-1e-5 band of both bounds (the exact double evaluation of correspondence_test is not what is under test here)
        mx = f32(p["inlier_curvature_ratio_threshold"]); mn = f32(1.0) / mx
        est = (t["rc"] + f32(1e-5)) / (t["cc"] + f32(1e-5))
        assert ((est > mn * (f32(1) + f32(1e-5))) & (est < mx * (f32(1) - f32(1e-5)))).all(), case.name
        cc = case.cur["curvature"][t["ci"]]; rc = case.ref["curvature"][t["ri"]]
        u = A.ulps(cc, thr)
        cover = {"current curvature at cls_thr exactly": int((cc == thr).sum()), "current curvature below cls_thr": int((cc < thr).sum()),
                 "current curvature above cls_thr": int((cc > thr).sum()), "reference curvature on the other side": int(((cc < thr) != (rc < thr)).sum()),
                 "reference curvature 1 .. 3 ulps across": int((((cc < thr) != (rc < thr)) & (np.abs(A.ulps(rc, thr)) <= 3)).sum())}
        assert set(np.unique(u).tolist()) == set(range(-4, 5)), case.name
        for k, floor in (("current curvature at cls_thr exactly", 50), ("current curvature below cls_thr", 100), ("current curvature above cls_thr", 100),
                         ("reference curvature on the other side", 100), ("reference curvature 1 .. 3 ulps across", 50)):
            assert cover[k] >= floor, (case.name, k, cover[k])
            total[k] = total.get(k, 0) + cover[k]
        assert ((sub == "across") == ((cc < thr) != (rc < thr))).all()
        # the uploaded form of the case carries the shipped table by the same rule
        assert np.array_equal(case.cur["omega_n"], FC.omega_n_by_rule(case.cur, FC.TABLES["shipped"], case.cls_thr))
        # wrong rules, each against the right one with the rotated table: the model's H moves by more than the GPU test's bar in some entry
        Tinv = O.iso_inverse(case.guess)
        right = FC.omega_n_by_rule(case.cur, rot, case.cls_thr)
        H, b, Habs, babs = _model_H(ra, ca, corr, Tinv, p, right)
        barH, barb = A.hb_bar(Habs, babs, H, b, max(A.CHAIN, 8))
        flat = f32(p["flat_curvature_threshold"])
        ref_curv = np.zeros(len(case.cur["curvature"]), f32); ref_curv[corr[:, 1]] = case.ref["curvature"][corr[:, 0]]
        wrong = {"<= in the class test": FC.omega_n_of_classes(FC.classes_by_rule(case.cur, case.cls_thr, less=np.less_equal), rot),
                 "classed by the reference's curvature": FC.omega_n_of_classes(FC.classes_by_rule(case.cur, case.cls_thr, curvature=ref_curv), rot),
                 "table rows swapped": FC.omega_n_by_rule(case.cur, rot[::-1], case.cls_thr)}
        if case.cls_thr <= p["flat_curvature_threshold"]:      # above flatThr the finder's clamp leaves curvatures near cls_thr alone: the same classes
            wrong["classed by the clamped curvature"] = FC.omega_n_of_classes(FC.classes_by_rule(case.cur, case.cls_thr, curvature=np.maximum(case.cur["curvature"], flat)), rot)
        for name, on in wrong.items():
            Hw, bw, _, _ = _model_H(ra, ca, corr, Tinv, p, on)
            frac = float((np.abs(Hw - H) / np.maximum(barH, 1e-300)).max())
            print(f"  {case.name:34s} {name:40s} moves H by {frac:10.1f} of the bar")
            assert frac > 1.0, (case.name, name, frac)
            total["min " + name] = min(total.get("min " + name, np.inf), frac)
        # A transposed read of the table is NOT told apart by H and b: the mirror entries of a table rounded entry by entry differ in their
        # last bits only, every term moves by that much, and the bar allows 14 roundings of the sum of the magnitudes.  Measured: at most
        # 0.0052 of the bar.  Recorded here as what it is; the host's expansion of the table is held bit for bit by the GPU test's downloads.
        Ht, bt, _, _ = _model_H(ra, ca, corr, Tinv, p, FC.omega_n_by_rule(case.cur, rot.transpose(0, 2, 1), case.cls_thr))
        ft = float((np.abs(Ht - H) / np.maximum(barH, 1e-300)).max())
        total["max transposed table"] = max(total.get("max transposed table", 0.0), ft)
        assert not np.array_equal(Ht, H) and ft < 0.05, (case.name, ft)
    for k, v in total.items():
        print(f"  {k:50s} {v}")


def test_step_distance_on_converter_form_cases(oracle):
    """as test_step_distance_of_the_oracle, on the cases and (threshold, table) pairs the GPU test runs in the converter's form"""
    worst, where = 0.0, None
    for case, thr, tname in A.converter_form_cases():
        ra, ca = FC.oracle_arrays(case, "exact9", FC.TABLES[tname], thr)
        mk = lambda a: oracle.Cloud.from_arrays(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])
        oref, ocur = mk(ra), mk(ca)
        for over in ({}, {"robust_kernel": 0}):
            d, _ = A.step_distance(oracle, M, case, ra, ca, oref, ocur, **over)
            if d > worst:
                worst, where = d, (case.name, thr, tname, over)
    print(f"worst oracle-to-float64 step distance on the converter-form cases {worst:.3e} at {where}")
    assert worst <= CONVERTER_FORM_STEP_DISTANCE
