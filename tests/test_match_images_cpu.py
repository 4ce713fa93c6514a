"""tests/match_images.py without a GPU: the integer model of the matchClouds score against the oracle (pwn_matcher_base.cpp:153-182) on every
built pair -- counts exact; distance bit for bit where the sum of the masked differences stays at or below 2^18 mm, within (n - 1) 2^-24 for
the long sum, NaN for the empty pair -- and the conditions the builder promises: every class of the bitwise-and occurs, holes on either and on
both sides, the tail pair's two pixels, the sum bounds, distinct scores within a batch, and frames that survive unProject + project."""
from fractions import Fraction

import numpy as np
import pytest

import match_images as MI

THRESHOLDS = (50.0, 2.5, 3.0, 0.0)


def _all_pairs():
    return MI.batch_pairs(20) + [MI.single_pair(), MI.table_pair()]


def check_against_oracle(oracle, kind, model, o, n_common):
    """a model score against the oracle's on the same images: what every test of these pairs asserts"""
    assert (model["nonZeros"], model["inliers"], model["outliers"]) == (o["image_nonZeros"], o["image_inliers"], o["image_outliers"])
    od = np.float32(o["image_reprojectionDistance"])
    if kind == "empty":
        assert np.isnan(model["distance"]) and np.isnan(od)
    elif kind == "long":
        assert abs(float(model["distance"]) - float(od)) <= MI.long_sum_bar(n_common) * float(od), (float(model["distance"]), float(od))
    else:
        assert MI.same_distance(model["distance"], od), (float(model["distance"]), float(od))


def test_batches_are_prefixes_of_one_list():
    for n in (3, 9):
        assert [p.name for p in MI.batch_pairs(n)] == [p.name for p in MI.batch_pairs(20)][:n]
    assert len({p.name for p in MI.batch_pairs(20)}) == 20


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_model_equals_the_oracle(oracle, threshold):
    for p in _all_pairs():
        m = MI.score(p.ref, p.cur, threshold)
        o = oracle.match_score(p.ref, p.cur, threshold)
        check_against_oracle(oracle, p.kind, m, o, m["nonZeros"])
        if threshold == 0.0:
            assert m["inliers"] == 0, p.name                           # strict `<`


def test_classes_holes_and_sum_bounds():
    n_long = 0
    for p in _all_pairs():
        cl = MI.classes(p.ref, p.cur)
        s = MI.score(p.ref, p.cur, 50.0)
        assert sum(cl.values()) == s["nonZeros"], p.name
        rz, cz = MI.to_u16(p.ref) == 0, MI.to_u16(p.cur) == 0
        if p.kind in ("bitwise", "long"):
            assert all(cl[c] >= 1 for c in MI.CLASSES), (p.name, cl)
            if p.name.startswith(("bitwise/", "long/")):
                assert (rz & ~cz).sum() > 0 and (~rz & cz).sum() > 0 and (rz & cz).sum() > 0, p.name
            i25, i30, i50 = (MI.score(p.ref, p.cur, t)["inliers"] for t in (2.5, 3.0, 50.0))
            assert 0 < i25 < i30 < i50 < s["nonZeros"], p.name          # 2.5 and 3.0 separate values the mask creates (5 -> 2.5, 3 -> 3)
        if p.kind == "long":
            n_long += 1
            assert s["sum_mm"] > MI.BITWISE_SUM_MM, p.name
            s64, ones = MI.sum64(p.ref, p.cur)                          # the 1 mm pixels decide the last bit of this sum
            assert MI.is_tie(s64, down=True) and ones >= 1 and MI.f32_of(Fraction(s64, 64)) != MI.f32_of(s["sum_units"] * MI.UNIT)
        else:
            assert s["sum_mm"] <= MI.BITWISE_SUM_MM, (p.name, s["sum_mm"])
        if p.kind == "one_mm":
            assert cl["1"] >= 1 and cl["0"] >= 1 and cl["0"] + cl["1"] == s["nonZeros"], cl
            assert s["sum_units"] == cl["1"] and s["distance"] == np.float32(np.float32(np.ldexp(float(cl["1"]), -MI.TINY_EXP)) / np.float32(s["nonZeros"]))
            assert s["inliers"] == s["nonZeros"]
        if p.kind == "tail":
            n = p.ref.size
            common = np.flatnonzero(~rz.reshape(-1) & ~cz.reshape(-1))
            assert len(common) == 2 and common[1] == n - 1 and (n // MI.WG) * MI.WG <= common[0] < n - 1
            assert (~cz).sum() == 2 and (~rz).sum() == n                # a current cloud much smaller than its reference
        if p.kind == "empty":
            assert s["nonZeros"] == 0 and (~rz).sum() > 0 and (~cz).sum() > 0
        if "/tail" in p.name:                                           # holes over the last rows: the tail workgroups contribute nothing
            assert rz.reshape(-1)[-(p.ref.size % MI.WG) - MI.WG:].all(), p.name
    assert n_long == 1
    assert (MI.BATCH_SHAPE[0] * MI.BATCH_SHAPE[1]) % MI.WG != 0          # the batched image ends in the middle of a workgroup
    assert MI.BATCH_SHAPE[0] * MI.BATCH_SHAPE[1] > 64 * MI.WG and MI.SINGLE_SHAPE[0] * MI.SINGLE_SHAPE[1] > 256 * MI.WG


def test_scores_within_a_batch_are_distinct():
    for n in (3, 9, 20):
        keys = []
        for p in MI.batch_pairs(n):
            s = MI.score(p.ref, p.cur, 50.0)
            keys.append((s["nonZeros"], s["inliers"], s["sum_units"]))
        assert len(set(keys)) == n, keys
        sizes = [int((MI.to_u16(p.cur) > 0).sum()) for p in MI.batch_pairs(n)] + [int((MI.to_u16(p.ref) > 0).sum()) for p in MI.batch_pairs(n)]
        assert len(set(sizes)) >= n                                     # clouds of different point counts


def test_frames_survive_unproject_and_project(oracle):
    """under an identity guess the finder's images are the frames: every valid pixel's point projects back onto that pixel, depth bit for bit"""
    for p in (MI.batch_pairs(20)[0], MI.batch_pairs(20)[2], MI.batch_pairs(20)[4], MI.single_pair(), MI.table_pair()):
        rows, cols = p.ref.shape
        K = MI.camera(rows, cols)
        cp = oracle.converter_params(K=K, **MI.converter_conf())
        for frame in (p.ref, p.cur):
            pts, idx = oracle.unproject(cp, frame)
            assert len(pts) == int((frame > 0).sum())
            pi, pd = oracle.project(K, np.eye(4), MI.MIN_DISTANCE, MI.MAX_DISTANCE, rows, cols, pts)
            assert np.array_equal(pi, idx) and np.array_equal(pi >= 0, frame > 0), p.name
            assert np.array_equal(pd[frame > 0].view(np.uint32), frame[frame > 0].view(np.uint32)), p.name
            assert np.array_equal(MI.to_u16(pd), MI.to_u16(frame))


def test_float32_rounding_of_exact_sums():
    rng = np.random.default_rng(3)
    for _ in range(200):
        k = int(rng.integers(1, 1 << 40)); e = int(rng.integers(-120, 20))
        want = np.float32(np.ldexp(np.float64(k), e)) if k < (1 << 53) else None
        assert MI.bits(MI.f32_of(Fraction(k) * Fraction(2) ** e)) == MI.bits(want)
    tie = Fraction((1 << 24) + 1, 64)                                   # half-way between two floats: to even ...
    assert MI.f32_of(tie) == np.float32((1 << 24) / 64.0)
    assert MI.f32_of(tie + MI.UNIT) == np.float32(((1 << 24) + 2) / 64.0)  # ... unless a 1 mm pixel tips it
