"""The injected projection points (tests/project_points.py) without a GPU: the numpy model against the oracle, word for word; every label met in
the oracle's images; every wrong-projection variant of the model visible on the injected set; the host's single-point form
(pwn_hip_project_point) against the model on every injected point; the testing entry point's null check."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_points as PP      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def cases(oracle):
    return PP.all_cases()


def test_summary_of_the_injected_set(cases, capsys):
    """per family: points, decisions made by rounding; per variant: pixels it changes (printed, so that a run shows what the set holds)"""
    lines = PP.summary(cases)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    rounding = {line.split(":")[0]: int(line.split(" points, ")[1].split(" ")[0]) for line in lines if " points, " in line}
    assert rounding["round_tie"] >= PP.REPEAT and rounding["depth_edge"] >= PP.REPEAT


def test_model_equals_oracle_on_every_case(cases, oracle):
    for c in cases:
        mi, md = PP.model_images(c)
        if not c.ask_oracle:
            ei, ed = PP.empty_images(c)
            assert np.array_equal(mi, ei) and np.array_equal(PP.bits(md), PP.bits(ed)), c.name      # far: the model rejects every point
            continue
        oi, od = oracle.project(c.K, c.T, c.min_d, c.max_d, c.rows, c.cols, c.points4())
        assert np.array_equal(mi, oi) and np.array_equal(PP.bits(md), PP.bits(od)), PP.describe_difference(c, mi, md, oi, od)


def test_the_models_own_variant_code_is_the_model(cases):
    """project(variant=...) shares everything but the varied line with a restatement of numpy_reference_model.project: with nothing varied
    it returns that function's words"""
    for c in cases:
        mi, md = PP.model_images(c)
        vi, vd = PP.project(c.P, PP.krt(c), c.min_d, c.max_d, c.rows, c.cols, variant="none")
        assert np.array_equal(mi, vi) and np.array_equal(PP.bits(md), PP.bits(vd)), c.name


def test_labels_are_met_in_the_oracles_images(cases, oracle):
    """the share that may miss is 0: a tie lands where roundf puts it, a rejected label is nowhere, a group's winner is the labelled point"""
    expectations = 0
    for c in cases:
        idx = oracle.project(c.K, c.T, c.min_d, c.max_d, c.rows, c.cols, c.points4())[0] if c.ask_oracle else PP.model_images(c)[0]
        unmet = PP.unmet_labels(c, idx)
        assert not unmet, (c.name, len(unmet), unmet[:8])
        expectations += int((c.expect != PP.OPEN).sum())
    assert expectations > 3000


def test_every_label_has_its_points(cases):
    """REPEAT points per sub label of the exact cases (a collide group: as many as its label says), one per ladder step"""
    for c in cases:
        fam = c.name.split("/")[0]
        if c.guess != "identity" or fam in ("collide", "far"):
            continue
        subs, counts = np.unique(c.sub[c.family == fam].astype(str), return_counts=True)
        assert len(subs) and (counts >= PP.REPEAT).all(), (c.name, dict(zip(subs, counts)))
    ties = [c for c in cases if c.name.startswith("round_tie") and c.guess == "identity"]
    for cam, (rows, cols, _) in PP.CAMERAS.items():
        subs = set(s for c in ties if c.camera == cam for s in c.sub)
        for axis, size in (("col", cols), ("row", rows)):
            for t in PP.tie_targets(size):
                assert f"{axis}{t:g}/tie" in subs, (cam, axis, t)
                assert any(s.startswith(f"{axis}{t:g}/below(") for s in subs) and any(s.startswith(f"{axis}{t:g}/above(") for s in subs), (cam, axis, t)
    col = PP.case_named("collide/wide")
    for m in PP.GROUPS:
        for kind in ("equal", "near_high", "near_low"):
            assert int((col.sub == f"{kind}{m}").sum()) == m
    g = col.group[np.nonzero(col.sub == "own_thread/near_last")[0][0]]
    idx = np.nonzero(col.group == g)[0]
    assert list(idx - idx[0]) == [0, 256, 512, 768] and col.P[idx[3], 2] == col.P[idx, 2].min() and col.expect[idx[3]] == PP.PRESENT
    idx = np.nonzero(col.sub == "one_wave/near_high")[0]
    assert len(idx) == 64 and idx[0] % 64 == 0 and idx[-1] - idx[0] == 63 and col.expect[idx[-1]] == PP.PRESENT
    idx = np.nonzero(col.sub == "cross_wg/near_high")[0]
    assert (np.diff(idx) > 1024).all() and col.expect[idx[-1]] == PP.PRESENT
    assert [c.n for c in cases if c.name.startswith("sizes")] == list(PP.SIZES)


@pytest.mark.parametrize("variant", PP.VARIANTS)
def test_every_wrong_projection_shows_on_the_injected_set(cases, variant):
    n = PP.variant_count(variant, cases)
    print(f"variant {variant}: {n} pixels changed")
    assert n >= PP.REPEAT, (variant, n)


def test_single_point_form_on_every_injected_point(cases):
    """pwn_hip_project_point (host code of the product library): acceptance, the depth's bits and the rounded pixel are the model's, before
    the model's image-bounds test; a coordinate an int cannot hold comes back saturated, a NaN as INT_MIN"""
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    x, y, d = C.c_int(0), C.c_int(0), C.c_float(0)
    for c in cases:
        ok, dm, fx, fy = PP.single_points(c)
        Kc = np.array([c.K[0], 0, 0, 0, c.K[1], 0, c.K[2], c.K[3], 1], F)
        Tc = np.ascontiguousarray(np.asarray(c.T, F).T.reshape(-1))
        P = np.ascontiguousarray(c.P, F)

        def want(f):
            if np.isnan(f):
                return PP.INT_MIN
            return int(min(max(float(f), -PP.SATURATED), PP.SATURATED))
        for i in range(c.n):
            got = L.pwn_hip_project_point(Kc.ctypes.data, Tc.ctypes.data, c.min_d, c.max_d, P[i].ctypes.data, C.byref(x), C.byref(y), C.byref(d))
            assert bool(got) == bool(ok[i]), (c.name, c.label(i))
            assert np.float32(d.value).view(np.uint32) == dm[i].view(np.uint32), (c.name, c.label(i))
            if got:
                assert (x.value, y.value) == (want(fx[i]), want(fy[i])), (c.name, c.label(i), x.value, y.value, fx[i], fy[i])
    far = PP.case_named("far/wide")
    ok, dm, fx, fy = PP.single_points(far)
    with np.errstate(invalid="ignore"):
        assert (ok & ((np.abs(fx) >= 2.0 ** 31) | (np.abs(fy) >= 2.0 ** 31))).sum() >= PP.REPEAT and (ok & (np.isnan(fx) | np.isnan(fy))).sum() >= 4


def test_testing_entry_point_refuses_a_null_context_and_stays_out_of_the_boundary():
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    g = C.c_int(-7)
    assert L.pwn_hip_debug_project_pairs(None, None, 1, None, None, 0, 0, None, None, C.byref(g)) == 1 and g.value == -7
    assert L.pwn_hip_last_error_string(None)
    assert "debug_" not in open(os.path.join(ROOT, "include", "pwn_hip.h")).read()
    assert "pwn_hip_debug_project_pairs" in open(os.path.join(ROOT, "include", "pwn_hip_testing.h")).read()


def test_batches_hold_nine_cases_of_one_image(cases):
    bs = PP.batches(cases)
    assert all(len(b) == 9 and len(set(c.key for c in b)) == 1 for b in bs)
    assert set(id(c) for b in bs for c in b) == set(id(c) for c in cases)
    sizes = [b for b in bs if b[0].name.startswith("sizes")]
    assert len(sizes) == 1 and [c.n for c in sizes[0]] == list(PP.SIZES)
    assert len(set(PP.bits(c.T).tobytes() for c in sizes[0])) == 9      # nine different transforms in the one launch
