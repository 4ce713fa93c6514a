"""The merged closure without a GPU: the numpy model of Merger2::mergeDepthImage (tests/merged_partition.py) in its two forms, the coverage
of the inputs the GPU tests compare the kernels on, and the host algebra of the PwnCloserWithMerger mirror."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merged_partition as M      # noqa: E402

SHAPES = [(1, 1), (1, 65), (7, 63), (9, 65), (17, 129), (60, 80)]


def same(a, b):
    return (np.array_equal(M.bits(a[0]), M.bits(b[0])) and np.array_equal(M.bits(a[1]), M.bits(b[1])) and np.array_equal(a[2], b[2]) and a[3] == b[3])


@pytest.fixture(scope="module")
def natural(oracle):
    return M.natural_case()


def test_vectorised_model_equals_the_literal_loop_on_injected_planes():
    for rows, cols in SHAPES:
        for n in (1, 2, 9):
            c = M.injected_case(rows, cols, n)
            assert same(M.merge_images(c["out"], c["weights"], c["planes"]), M.merge_images_literal(c["out"], c["weights"], c["planes"])), (rows, cols, n)


def test_vectorised_model_equals_the_literal_loop_on_natural_planes(natural):
    z = np.zeros((natural["rows"], natural["cols"]), np.float32)
    assert same(M.merge_images(z, z, natural["planes"]), M.merge_images_literal(z, z, natural["planes"]))
    # n images in one call are n successive calls, and a split call continues where the first part stopped
    a = M.merge_images(z, z, natural["planes"][:3])
    b = M.merge_images(a[0], a[1], natural["planes"][3:])
    full = M.merge_images(z, z, natural["planes"])
    assert np.array_equal(M.bits(b[0]), M.bits(full[0])) and np.array_equal(M.bits(b[1]), M.bits(full[1])) and a[3] + b[3] == full[3]


def test_natural_case_takes_every_branch_often_enough(natural):
    """60 x 80, K = (65.6, 65.6, 39.5, 29.5), seed 3, eight clouds.  Measured with the oracle: 4 552 first writes, 10 084 nearer-replacements,
    15 094 fusions, 505 ignored beyond 0.2, 21 pixels within 1e-6 of the -3e-5 threshold, overlap counts 3 427 .. 4 388 (pairwise distinct),
    210 fusions a fused multiply-add of the first product rounds differently, 1 842 a reciprocal multiply does."""
    z = np.zeros((natural["rows"], natural["cols"]), np.float32)
    _, _, overlap, points, st = M.merge_images(z, z, natural["planes"])
    print(st, overlap.tolist(), points)
    assert st["first"] >= 1000 and st["nearer"] >= 1000 and st["fused"] >= 1000 and st["beyond"] >= 100
    assert st["near_threshold"] >= 5
    assert len(set(overlap.tolist())) == len(overlap)
    assert st["fma_differs"] >= 50 and st["fma2_differs"] >= 50 and st["rcp_differs"] >= 500
    assert points == st["first"] + st["nearer"]
    # a wrongly rounded kernel also ends with another image: pixels of the FINAL fused image that differ from the right one (a wrong rounding
    # is often overwritten by a later nearer-replacement, so these are fewer than the fusions above: measured 65 / fma, 486 / rcp)
    right = M.merge_images(z, z, natural["planes"])[0]
    final = {v: int((M.bits(M.merge_images(z, z, natural["planes"], variant=v)[0]) != M.bits(right)).sum()) for v in ("fma", "fma2", "rcp")}
    print(final)
    assert min(final.values()) >= 50


def test_injected_labels_sit_on_both_sides_of_every_branch():
    c = M.injected_case(17, 129, 1)
    out0, w0, d = c["out"].reshape(-1), c["weights"].reshape(-1), c["planes"][0].reshape(-1)
    out1, w1, _, _, _ = M.merge_images(c["out"], c["weights"], c["planes"])
    out1, w1 = out1.reshape(-1), w1.reshape(-1)
    changed = M.bits(out1) != M.bits(out0)
    taken = {}
    for name, pix in c["label_pixels"].items():
        assert len(pix) >= M.REPEAT, name
        state = set(bool(changed[i]) or M.bits(w1)[i] != M.bits(w0)[i] for i in pix)
        assert len(state) == 1, name                      # every pixel of a label takes the same branch
        taken[name] = state.pop()
    # the selection test: nothing at or below 0.1 / at or above 10000 is taken, the neighbours inside are
    for fill in ("fresh", "filled"):
        assert [taken["lo%+d/%s" % (k, fill)] for k in (-2, -1, 0, 1, 2)] == [False, False, float(np.float32(0.1)) > 0.1, True, True]
        assert [taken["hi%+d/%s" % (k, fill)] for k in (-2, -1, 0, 1, 2)] == [True, True, False, False, False]
        for name in ("zero", "neg_zero", "negative", "denormal", "flt_max", "pos_inf", "neg_inf", "nan"):
            assert not taken["%s/%s" % (name, fill)], name
    # d - out around -3e-5 on a filled pixel: replaced (out becomes d) below the threshold, fused above it
    for k in (-2, -1, 0, 1, 2):
        i = c["label_pixels"]["nearer%+d/filled" % k][0]
        replaced = M.bits(out1)[i] == M.bits(d)[i]
        assert replaced == (float(np.float32(d[i] - out0[i])) < -.00003), k
    assert {M.bits(out1)[c["label_pixels"]["nearer%+d/filled" % k][0]] == M.bits(d)[c["label_pixels"]["nearer%+d/filled" % k][0]] for k in (-2, -1, 0, 1, 2)} == {True, False}
    # |d - out| around 0.2 on both sides of out: fused inside, left alone outside
    for sign in "+-":
        got = [taken["fuse%s%+d/filled" % (sign, k)] for k in (-2, -1, 0, 1, 2)]
        want = [float(np.abs(np.float32(d[c["label_pixels"]["fuse%s%+d/filled" % (sign, k)][0]] - np.float32(1.5)))) < .2 or
                float(np.float32(d[c["label_pixels"]["fuse%s%+d/filled" % (sign, k)][0]] - np.float32(1.5))) < -.00003 for k in (-2, -1, 0, 1, 2)]
        assert got == want
    assert [taken["fuse+%+d/filled" % k] for k in (-2, -1, 0, 1, 2)] == [True, True, False, False, False]


# ---------------------------------------------------------------------------------------------- the closer's host algebra (the mirror)
def rot(axis, deg):
    a = np.deg2rad(deg); c, s = np.cos(a), np.sin(a)
    R = np.eye(4)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R[i, i] = c; R[i, j] = -s; R[j, i] = s; R[j, j] = c
    return R


def pose(axis, deg, t):
    T = rot(axis, deg); T[:3, 3] = t
    return T


def test_som_is_an_integer_division_and_never_zero():
    from g2o_frontend_amd import api
    assert [api.PwnCloserWithMerger.som(n) for n in (0, 1, 7, 8, 15, 16, 17, 128)] == [1, 1, 1, 1, 1, 2, 2, 16]
    assert [M.som_of(n) for n in (0, 1, 7, 8, 15, 16, 17, 128)] == [1, 1, 1, 1, 1, 2, 2, 16]


def test_rejection_rule_uses_integer_halves_and_eighths():
    from g2o_frontend_amd import api

    def rejects(nz, out, inl, minNonZero=3000, minInliers=1000):
        closer = api.PwnCloserWithMerger.__new__(api.PwnCloserWithMerger)
        closer._frameMinNonZeroThreshold, closer._frameMinInliersThreshold = minNonZero, minInliers
        got = closer.rejects(dict(image_nonZeros=nz, image_outliers=out, image_inliers=inl))
        assert got == M.rejected(nz, out, inl, minNonZero, minInliers)
        return got
    # inliers / 8 truncates: 7 -> 0, 8 -> 1, 15 -> 1 (hand-computed); the other two tests switched off by thresholds of 0
    assert rejects(5000, 0, 7, 0, 0) is False and rejects(5000, 1, 7, 0, 0) is True
    assert rejects(5000, 1, 8, 0, 0) is False and rejects(5000, 2, 8, 0, 0) is True
    assert rejects(5000, 1, 15, 0, 0) is False and rejects(5000, 2, 15, 0, 0) is True
    # 3001 / 2 = 1500 and 1001 / 2 = 500: the odd thresholds lose their half
    assert rejects(1500, 0, 800, 3001, 0) is False and rejects(1499, 0, 800, 3001, 0) is True
    assert rejects(5000, 0, 500, 0, 1001) is False and rejects(5000, 0, 499, 0, 1001) is True
    # the defaults: 1500 non-zeros, 500 inliers, outliers <= inliers / 8
    assert rejects(1500, 62, 500) is False and rejects(1500, 63, 500) is True and rejects(1499, 0, 500) is True and rejects(1500, 0, 499) is True


def test_projector_transform_and_relation_fan_out_against_hand_computed_values():
    from g2o_frontend_amd import api
    # quarter turns and whole-number translations: every product is exact in float64, so the hand-computed matrices are too
    current = api.MapNode("c", pose(2, 90, (1, 2, 3)))
    other = api.MapNode("o", pose(0, 90, (4, 0, -1)))
    offset = pose(1, 90, (0, 1, 0))
    for T in (current.transform(), other.transform(), offset):
        T[np.abs(T) < 1e-12] = 0.0
    tr = api.PwnCloserWithMerger.projectorTransform(other, current, offset)
    # other^-1 = [Rx(-90) | -Rx(-90) t], by hand: R = [[1,0,0],[0,0,1],[0,-1,0]], t = (-4, 1, 0)
    inv_other = np.array([[1, 0, 0, -4], [0, 0, 1, 1], [0, -1, 0, 0], [0, 0, 0, 1]], np.float64)
    want = inv_other @ current.transform() @ offset
    # inv_other * current = [[0,-1,0,-3],[0,0,1,4],[-1,0,0,-2]]; times the offset [Ry(90) | (0,1,0)]:
    by_hand = np.array([[0, -1, 0, -4], [-1, 0, 0, 4], [0, 0, -1, -2], [0, 0, 0, 1]], np.float64)
    assert np.array_equal(want, by_hand)
    assert tr.dtype == np.float32 and np.array_equal(tr, want.astype(np.float32))
    assert np.array_equal(tr, M.projector_transform(other.transform(), current.transform(), offset))
    # fan-out: nodo2 = current gives result * current^-1 * nodo, moved into current's frame
    result = pose(1, 90, (0, 0, 2)); result[np.abs(result) < 1e-12] = 0.0
    got = api.PwnCloserWithMerger.relationTransform(current, current, result, other)
    inv_current = np.array([[0, 1, 0, -2], [-1, 0, 0, 1], [0, 0, 1, -3], [0, 0, 0, 1]], np.float64)       # Rz(-90), -Rz(-90) t by hand
    assert np.array_equal(inv_current @ current.transform(), np.eye(4))
    want = inv_current @ current.transform() @ result @ inv_current @ other.transform()
    # = result * (current^-1 * other) = [Ry(90) | (0,0,2)] * [[0,0,-1,-2],[-1,0,0,-3],[0,1,0,-4]]
    by_hand = np.array([[0, 1, 0, -4], [-1, 0, 0, -3], [0, 0, 1, 4], [0, 0, 0, 1]], np.float64)
    assert np.array_equal(want, by_hand) and np.array_equal(got, by_hand)
    assert np.allclose(got, M.relation_transform(current.transform(), current.transform(), result, other.transform()), atol=1e-12)
    # general poses: the loops of the mirror against numpy's products
    rng = np.random.default_rng(4)
    for _ in range(20):
        A, B, Cc = (pose(int(rng.integers(3)), rng.uniform(-170, 170), rng.normal(size=3)) @ pose(int(rng.integers(3)), rng.uniform(-170, 170), rng.normal(size=3))
                    for _ in range(3))
        a, b = api.MapNode("a", A), api.MapNode("b", B)
        assert np.allclose(api.PwnCloserWithMerger.projectorTransform(a, b, Cc), M.projector_transform(A, B, Cc), atol=1e-6)
        assert np.allclose(api.PwnCloserWithMerger.relationTransform(a, b, Cc, a), M.relation_transform(A, B, Cc, A), atol=1e-12)
    assert np.array_equal(api.PwnCloserWithMerger.INFORMATION, np.diag([100.0, 100, 100, 1000, 1000, 1000]))
    assert np.array_equal(M.INFORMATION, api.PwnCloserWithMerger.INFORMATION)


def test_new_entry_points_refuse_null_arguments_without_a_device():
    import ctypes as C
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    assert L.pwn_hip_merge_depth_images(None, 1, None, 4, 4, None, None, None, None) == 1
    assert L.pwn_hip_project_merge_batch(None, None, 1, None, None, 0.01, 6.0, 4, 4, None, None, None, None, None) == 1
    assert L.pwn_hip_last_error_string(None)
