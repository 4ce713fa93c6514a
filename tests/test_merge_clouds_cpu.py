"""The cloud-level fusion (Merger2::merge) without a GPU: the numpy model of tests/merge_clouds.py in its two forms, the coverage of the
inputs the GPU tests compare the kernels on, the host algebra of the PwnMerger mirror and the new entry point's null refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_clouds as MC      # noqa: E402
from conftest import case_params      # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def injected_total(c):
    return MC.total_from_arrays(c["total"], c["weights"])


def both_forms(total, clouds, transforms, proj, gauss=False):
    v = MC.merge_list(total, clouds, transforms, proj, gauss=gauss)
    lit = MC.merge_list_literal(total, clouds, transforms, proj, gauss=gauss)
    assert MC.same_total(v[0], lit[0]) and np.array_equal(v[1], lit[1]) and np.array_equal(v[2], lit[2])
    return v


@pytest.mark.parametrize("rows,cols", MC.SHAPES)
def test_vectorised_model_equals_the_literal_loop_on_injected_clouds(oracle, rows, cols):
    for n, ranges, moved in MC.injected_variants(rows, cols):
        c = MC.injected_case(rows, cols, n, ranges, moved)
        total, appended, fused, counts, _ = both_forms(injected_total(c), MC.oracle_clouds(c), c["transforms"], c["proj"])
        assert len(total["points"]) == len(c["total"]["points"]) + int(appended.sum()), (n, ranges, moved)
        assert all(k["drop_unproject"] == 0 for k in counts)      # the image holds only depths inside the projector's range (docs/parity.md)


@pytest.mark.parametrize("rows,cols,with_offset", [(60, 80, False), (60, 80, True), (120, 160, False)])
def test_vectorised_model_equals_the_literal_loop_on_natural_clouds(oracle, rows, cols, with_offset):
    case = MC.natural_case() if (rows, cols, with_offset) == (60, 80, False) else MC.natural_case(rows, cols, MC.K_SMALL if rows == 60 else case_params("small")[2],
                                                                                                  with_offset=with_offset)
    full = both_forms(MC.empty_total(gauss=True), case["clouds"], case["transforms"], case["proj"], gauss=True)
    # a list in one call is the same clouds in successive calls, and a split call continues where the first part stopped
    a = MC.merge_list(MC.empty_total(gauss=True), case["clouds"][:3], case["transforms"][:3], case["proj"], gauss=True)
    b = MC.merge_list(a[0], case["clouds"][3:], case["transforms"][3:], case["proj"], gauss=True)
    assert MC.same_total(b[0], full[0]) and a[1].tolist() + b[1].tolist() == full[1].tolist()
    # without Stats and Gaussians on the sources (uploaded clouds): the default Stats() under T
    if rows == 60 and not with_offset:
        bare = [MC.stripped(c) for c in case["clouds"][:3]]
        t = both_forms(MC.empty_total(), bare, case["transforms"][:3], case["proj"])[0]
        assert np.array_equal(MC.bits(t["points"]), MC.bits(a[0]["points"])) and np.array_equal(MC.bits(t["omega_p"]), MC.bits(a[0]["omega_p"]))
        assert not t["eigenvalues"].any() and not t["npoints"].any()
        k0 = int(a[1][0])
        assert np.array_equal(t["stats"][:k0], np.tile(MC.DEFAULT_STATS, (k0, 1)))                   # the big node: identity * identity
        assert np.allclose(t["stats"][k0:k0 + 5].reshape(-1, 4, 4).transpose(0, 2, 1), case["transforms"][1], atol=0)      # T * identity = T


NATURAL_FLOORS = {          # per merged cloud, clouds 1..8: at most half of the smallest measured count (docs/parity.md has the table)
    (60, 80): dict(append_new=160, fuse=2100),             # measured minima over clouds 1..8: 334 / 4 214
    (120, 160): dict(append_new=700, fuse=8400),           # 1 400 / 16 968
}


@pytest.mark.parametrize("rows,cols", [(60, 80), (120, 160)])
def test_natural_case_takes_the_actions_often_enough(oracle, rows, cols):
    """Counts per merged cloud of the three actions and the three drops, printed; floors of at most half the measured count for every action
    the room scene reaches with at least 200 pixels over the list.  Measured (clouds 0 .. 8; append_new / fuse / append_occluder /
    drop_unproject / drop_between / drop_depth) -- see the table in docs/parity.md.  The occluder append and the drop between the two
    thresholds are rare in the room (a few pixels per cloud at depth edges): the injected inputs cover them."""
    case = MC.natural_case() if rows == 60 else MC.natural_case(rows, cols, case_params("small")[2])
    _, appended, fused, counts, diff = MC.merge_list(MC.empty_total(gauss=True), case["clouds"], case["transforms"], case["proj"], gauss=True)
    for i, k in enumerate(counts):
        print(rows, cols, "cloud", i, [k[a] for a in MC.ACTIONS])
    print("pixels a wrong kernel would round / decide differently:", diff)
    assert counts[0]["append_new"] == appended[0] >= 0.9 * len(case["clouds"][0])      # the big node into the empty total
    assert counts[0]["fuse"] == 0 and fused[0] == 0
    floors = NATURAL_FLOORS[(rows, cols)]
    for k in counts[1:]:
        for a, floor in floors.items():
            assert k[a] >= floor, (a, k[a], floor)
        assert k["drop_unproject"] == 0
    assert sum(k["fuse"] for k in counts) >= 200 and sum(k["append_new"] for k in counts[1:]) >= 200
    assert diff["fma"] >= 50 and diff["rcp"] >= 50 and diff["column_order"] >= 50


@pytest.mark.parametrize("rows,cols,with_offset", [(60, 80, False), (60, 80, True), (120, 160, False)])
def test_a_converted_cloud_merged_alone_equals_cloud_add(oracle, rows, cols, with_offset):
    """Merged alone into an empty total, under its own sensor offset and camera, a converter-made cloud comes out as oracle.Cloud.add of it, row
    for row, wherever a point reprojects into its own pixel: the appended pixels in raster order are the cloud's points in their own order.
    At least nine points in ten do (the oracle alone: index images are bit-exact today)."""
    from oracle import oracle as O
    case = MC.natural_case(rows, cols, MC.K_SMALL if rows == 60 else case_params("small")[2], with_offset=with_offset)
    K, offset, mn, mx, _, _ = case["proj"]
    cp = O.converter_params(K, sensor_offset=offset if with_offset else None, **case["conf"])
    for k in (0, 4):
        src, T = case["clouds"][k], case["transforms"][4]                      # a non-identity T: Cloud::add transforms too
        own = O.convert(cp, case["frames"][k])[1]                              # the converter's index image: every point's own pixel
        total, appended, _, counts, _ = MC.merge_list(MC.empty_total(gauss=True), [src], [T], case["proj"], gauss=True)
        added = O.Cloud(); added.add(src, T)
        want, wg = added.arrays(stats=True), added.gaussians()
        idx_c, dep_c = O.project(K, offset, mn, mx, rows, cols, src.arrays()["points"])
        home = (own >= 0) & (idx_c == own)
        share = home.sum() / len(src)
        print(rows, cols, with_offset, k, "points that reproject into their own pixel: %d of %d" % (home.sum(), len(src)))
        assert share >= 0.9
        taken = counts[0]["image"] != 5                                        # pixels that appended (an empty total: nothing else happens)
        assert int(taken.sum()) == appended[0] == len(total["points"])
        pos = np.cumsum(taken.reshape(-1)).reshape(rows, cols) - 1             # row of the total a pixel appended
        rows_t, rows_s = pos[home & taken], own[home & taken]
        assert len(rows_t) >= 0.9 * len(src)
        for key in MC.CLOUD_KEYS:
            assert np.array_equal(MC.bits(total[key][rows_t]), MC.bits(want[key][rows_s])), key
        for key in MC.GAUSS_KEYS:
            assert np.array_equal(MC.bits(total["gauss"][key][rows_t]), MC.bits(wg[key][rows_s])), key
        assert np.array_equal(MC.raw_bits(total["weights"][rows_t]), MC.raw_bits(F(1) / dep_c[home & taken]))
        if home.sum() == len(src) == appended[0]:
            assert np.array_equal(MC.bits(total["points"]), MC.bits(want["points"]))


def test_omega_transform_is_the_oracles_product(oracle):
    """the float32 product the model uses under the identity, checked where the oracle does multiply: a non-identity T"""
    from oracle import oracle as O
    from g2o_frontend_amd import synth
    c = MC.injected_case(17, 129, 1)
    src = MC.oracle_clouds(c)[0]
    T = synth.v2t(np.array([0.1, -0.05, 0.2, 0.03, -0.02, 0.05])).astype(F)
    added = O.Cloud(); added.add(src, T)
    a, b = src.arrays(), added.arrays()
    assert not np.isfinite(a["omega_p"]).all()
    for key in ("omega_p", "omega_n"):
        assert np.array_equal(MC.bits(MC.omega_transform(T, a[key])), MC.bits(b[key])), key
    # under the identity: a matrix with a non-finite entry does not come back as it went in
    same = MC.omega_transform(MC.EYE, a["omega_p"])
    fin = np.isfinite(a["omega_p"]).all(1)
    assert np.array_equal(MC.bits(same[fin]), MC.bits(a["omega_p"][fin])) and np.isnan(same[~fin]).any()


def test_injected_labels_land_on_their_side_of_every_branch(oracle):
    for ranges in ("wide", "narrow"):
        c = MC.injected_case(17, 129, 1, ranges)
        assert all(len(p) >= MC.REPEAT for p in c["label_pixels"].values())
        _, _, _, counts, _ = MC.merge_list(injected_total(c), MC.oracle_clouds(c), c["transforms"], c["proj"])
        img = counts[0]["image"].reshape(-1)
        for name, pix in c["label_pixels"].items():
            got = {MC.ACTIONS[img[i]] for i in pix}
            assert got == {c["expect"][name]}, (ranges, name, got)
        want = {k: v for k, v in c["expect"].items()}
        ks = (-2, -1, 0, 1, 2)
        if ranges == "wide":      # float(0.2f) > 0.2 and float(100f) == 100: the float against the double literal
            assert [want["lo%+d/fresh" % k] for k in ks] == ["drop_depth"] * 2 + ["append_new"] * 3
            assert [want["hi%+d/filled" % k] for k in ks] == ["fuse"] * 2 + ["drop_depth"] * 3
        else:                     # the projector's own range is inclusive
            assert [want["min%+d/fresh" % k] for k in ks] == ["drop_depth"] * 2 + ["append_new"] * 3
            assert [want["max%+d/filled" % k] for k in ks] == ["fuse"] * 3 + ["drop_depth"] * 2
        for sign in "+-":
            got = [want["near%s%+d" % (sign, k)] for k in ks]
            assert set(got) == {"fuse", "drop_between"} and got[0] == "fuse" and got[-1] == "drop_between"
        got = [want["occluder%+d" % k] for k in ks]
        assert set(got) == {"append_occluder", "drop_between"} and got[0] == "append_occluder" and got[-1] == "drop_between"


def test_the_inputs_tell_every_wrong_kernel_apart(oracle):
    """each mutation of docs/parity.md, applied to the model, ends with another total on the injected 17 x 129 list of three and on the natural list"""
    c = MC.injected_case(17, 129, 3)
    clouds = MC.oracle_clouds(c)
    right = MC.merge_list(injected_total(c), clouds, c["transforms"], c["proj"])
    nat = MC.natural_case()
    nright = MC.merge_list(MC.empty_total(gauss=True), nat["clouds"][:3], nat["transforms"][:3], nat["proj"], gauss=True)
    print(right[4], nright[4])
    for v in ("fma", "rcp", "column_order", "occluder015"):
        wrong = MC.merge_list(injected_total(c), clouds, c["transforms"], c["proj"], variant=v)
        assert not MC.same_total(wrong[0], right[0]), v
        assert right[4][v] >= 50, (v, right[4][v])
    # the 0.15 test in float is no mutation at all: 0.15f lies ABOVE 0.15 (it rounds up), so no float sits in [0.15, 0.15f) and
    # |delta| < 0.15f decides every float as (double)|delta| < 0.15 does -- unlike 0.2f > 0.2 and -0.3f < -0.3, where the float form differs
    assert float(F(.15)) > .15 and float(np.nextafter(F(.15), F(0))) < .15
    assert float(F(.2)) > .2 and float(F(-.3)) < -.3
    wrong = MC.merge_list(injected_total(c), clouds, c["transforms"], c["proj"], variant="float015")
    assert MC.same_total(wrong[0], right[0]) and right[4]["float015"] == 0
    for v in ("fma", "rcp", "column_order"):
        wrong = MC.merge_list(MC.empty_total(gauss=True), nat["clouds"][:3], nat["transforms"][:3], nat["proj"], gauss=True, variant=v)
        assert not MC.same_total(wrong[0], nright[0]), v


# ------------------------------------------------------------------------------------------------------- the mirror's algebra
def test_node_transform_against_the_model_on_random_poses():
    from g2o_frontend_amd import api
    from test_merged_partition_cpu import pose
    rng = np.random.default_rng(11)
    big = api.MapNode("b", pose(2, 90, (1, 2, 3)))
    assert np.array_equal(api.PwnMerger.nodeTransform(big, big), np.eye(4, dtype=F))      # quarter turn, whole numbers: exact
    for _ in range(20):
        A, B = (pose(int(rng.integers(3)), rng.uniform(-170, 170), rng.normal(size=3)) @ pose(int(rng.integers(3)), rng.uniform(-170, 170), rng.normal(size=3))
                for _ in range(2))
        a, b = api.MapNode("a", A), api.MapNode("b", B)
        got = api.PwnMerger.nodeTransform(a, b)
        assert got.dtype == np.float32 and np.allclose(got, MC.node_transform(A, B), rtol=0, atol=1e-6)
        exact = api._iso_mul_d(api._iso_inverse_d(A), B)
        assert np.allclose(exact, np.linalg.inv(A) @ B, rtol=0, atol=1e-12)


def test_new_entry_point_refuses_null_arguments_without_a_device():
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    assert L.pwn_hip_merge_clouds(None, None, None, 1, None, None, 0.01, 6.0, 4, 4, None, None, None, None) == 1
    assert L.pwn_hip_last_error_string(None)


def test_new_symbol_is_declared_and_prototyped():
    from g2o_frontend_amd import _lib
    assert "pwn_hip_merge_clouds" in _lib.PROTOTYPES and len(_lib.PROTOTYPES["pwn_hip_merge_clouds"][1]) == 14
    header = open(os.path.join(ROOT, "include", "pwn_hip.h")).read()
    assert "int pwn_hip_merge_clouds(" in header and "merger2.cpp:106-183" in header
