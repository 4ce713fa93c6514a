"""The numpy model of the traversability image (tests/manifold_image.py; ManifoldVoronoiExtractor::process, pwn_tracker2/
manifold_voronoi_extractor.cpp:50-127) without a GPU: its two forms agree in every bit, every injected label takes the branch it was built
for, the natural frames populate the image and depend on the order of the clouds and of the points, every wrong model of the mutation list
changes the injected image -- and the one reordering that is claimed to be safe changes nothing.  Then the mirrors' names and defaults."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_image as M      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GRIDS = [(1, 1), (1, 7), (7, 1), (16, 16), (17, 16), (37, 53), (100, 100)]


def both_forms(rows, resolution, xs, ys, image=None):
    a, ia, branches = M.splat_literal(rows, resolution, xs, ys, image=image)
    b, ib, events, longest = M.splat(rows, resolution, xs, ys, image=image)
    assert a.dtype == np.uint16 and a.shape == (xs, ys)
    assert np.array_equal(a, b) and np.array_equal(ia, ib), (xs, ys, resolution)
    return a, ia, branches, events, longest


@pytest.mark.parametrize("xs,ys", GRIDS)
def test_the_two_forms_agree_on_the_injected_clouds(oracle, xs, ys):
    n = 31 if (xs, ys) == (37, 53) else 7
    case, rows = M.injected(xs, ys, 0.2, n)
    img, inside, _, events, longest = both_forms(rows, 0.2, xs, ys)
    assert inside.sum() > 0 and events > 0
    # from a pre-filled image (accumulate): both forms start from it
    rng = np.random.default_rng(5)
    start = rng.choice(np.array([30000, 65535, 9000, 9300, 12000, 0], np.uint16), (xs, ys))
    both_forms(rows, 0.2, xs, ys, image=start)
    # a list split in two, the second half on the image of the first, is the list
    first = M.splat(rows[:3], 0.2, xs, ys)[0]
    assert np.array_equal(M.splat(rows[3:], 0.2, xs, ys, image=first)[0], img)


@pytest.mark.parametrize("resolution", [0.05, 0.2])
def test_the_two_forms_agree_on_the_natural_frames(oracle, resolution):
    _, _, rows = M.natural()
    img, inside, _, events, longest = both_forms(rows, resolution, 100, 100)
    obstacles, heights = int((img == M.OBSTACLE).sum()), int(((img != M.OBSTACLE) & (img != M.UNTOUCHED)).sum())
    print("resolution %.2f: %d obstacle cells, %d height cells, %d events, largest run %d, inside %s" % (resolution, obstacles, heights, events, longest, inside.tolist()))
    if resolution == 0.05:
        assert obstacles >= 100 and heights >= 100


def test_the_natural_image_depends_on_both_orders(oracle):
    _, _, rows = M.natural()
    img = M.splat(rows, 0.05, 100, 100)[0]
    other = M.splat([rows[i] for i in (7, 6, 5, 4, 3, 2, 1, 0, 8)], 0.05, 100, 100)[0]
    backwards = M.splat([(P[::-1], N[::-1]) for P, N in rows], 0.05, 100, 100)[0]
    a, b = int((other != img).sum()), int((backwards != img).sum())
    print("cells that differ: clouds fed as 7..0, 8: %d; index order reversed: %d" % (a, b))
    assert a >= 10 and b >= 10
    diff = {v: int((M.splat(rows, 0.05, 100, 100, variant=v)[0] != img).sum()) for v in ("nearest", "fused_pz", "fused_xy", "floor", "le")}
    print(diff)
    assert diff["nearest"] >= 100


def test_every_label_lands_on_its_branch(oracle):
    case, rows = M.injected()
    assert case["exact"] and case["n"] == 31
    _, _, branches = M.splat_literal(rows, case["resolution"], case["xs"], case["ys"])
    per_label, taken = {}, {}
    for cloud, idx, label, expect in case["labels"]:
        got = M.BRANCHES[branches[cloud][idx]]
        per_label[label] = per_label.get(label, 0) + 1
        taken.setdefault(label.split("/")[0], set()).add(got)
        if expect is not None:
            assert got == expect, (label, cloud, idx, expect, got)
    # at least REPEAT points per label group; the edge labels come per position (two each), REPEAT and more per value of k
    groups = {}
    for label, k in per_label.items():
        key = re.sub(r"[+-]\d+$", "", label) if label.startswith("xy_edge") else label
        groups[key] = groups.get(key, 0) + k
    for want in ("fused_xy/0", "fused_xy/1", "fused_z", "height_tie/good", "height_tie/bad", "height_tie/plus1", "order/bad_first", "order/then_higher_good",
                 "order/then_lower_bad", "order/then_higher_bad", "order/later_cloud_bad", "order/far_bad", "normal/sq_zero", "normal/sq_0.05",
                 "normal/sq_tenth-1", "normal/sq_tenth", "normal/sq_tenth+1", "normal/nz-1", "normal/nz+0", "normal/nz+1", "normal/negative",
                 "wrap/minus1/fresh", "wrap/minus1/filled", "wrap/minus100/fresh", "wrap/below-65536/filled", "wrap/30001/fresh", "wrap/above65535/filled",
                 "xy_edge/0/negative", "xy_edge/1/negative", "xy_edge/0/0", "xy_edge/0/1", "xy_edge/0/36", "xy_edge/0/37", "xy_edge/1/0", "xy_edge/1/1",
                 "xy_edge/1/52", "xy_edge/1/53"):
        assert groups.get(want, 0) >= M.REPEAT, (want, groups.get(want))
    # both sides of every edge and threshold are populated
    edge = {}
    for cloud, idx, label, expect in case["labels"]:
        if label.startswith("xy_edge") and not label.endswith("negative"):
            edge.setdefault(re.sub(r"[+-]\d+$", "", label), set()).add(expect)
    for axis, size in ((0, case["xs"]), (1, case["ys"])):
        # a sum a few ulps below 0 truncates to 0: nothing around k = 0 leaves the grid; around k = size both sides do their thing
        assert edge["xy_edge/%d/0" % axis] == {"set_height"} and edge["xy_edge/%d/%d" % (axis, size)] == {"outside", "set_height"}
    assert taken["normal"] >= {"norm_skip", "set_obstacle", "set_height"} and taken["wrap"] >= {"below_skip", "set_height", "obstacle_skip"}
    assert taken["crowd"] >= {"below_skip", "set_height", "set_obstacle"}
    # the far pair is another sort chunk apart, the crowd is one cell of one cloud, every cloud reaches the shared cell
    far = {label: [i for c, i, l, _ in case["labels"] if l == label] for label in ("order/far_good", "order/far_bad")}
    assert min(far["order/far_bad"]) - max(far["order/far_good"]) >= 2049
    assert per_label["crowd/one_cloud"] >= 5000 and per_label["crowd/every_cloud"] == 31
    x, y, inside, _, normal, _ = [np.concatenate(v) for v in zip(*[M.events(P, N, case["resolution"], case["xs"], case["ys"]) for P, N in rows])]
    last = np.cumsum([len(P) for P, _ in rows]) - 1                         # the shared cell's point closes every cloud
    assert len({(int(x[i]), int(y[i])) for i in last}) == 1 and inside[last].all() and normal[last].all()
    sizes = sorted({len(P) for P, _ in rows[2:]})
    assert sizes == sorted(M.SIZES)
    # squared norms: the floats around 0.1f in every bit, decided in double
    tenth = F(0.1)
    for t, passes in ((M._ulps(tenth, -1), False), (tenth, True), (M._ulps(tenth, 1), True)):
        nx, ny, nz = M.normal_with_squared_norm(t)
        assert ((nx * nx + ny * ny) + nz * nz) + F(0) == t and (not float(t) < 0.1) == passes


def test_every_wrong_model_changes_the_injected_image(oracle):
    case, rows = M.injected()
    args = (rows, case["resolution"], case["xs"], case["ys"])
    img = M.splat(*args)[0]
    diff = {}
    for v in M.VARIANTS:
        wrong = M.splat_literal(*args, variant=v)[0] if v == "norm_first" else M.splat(*args, variant=v)[0]
        diff[v] = int((wrong != img).sum())
    print(diff)
    for v, d in diff.items():
        if v == "norm_first":      # the norm test before the height test: both only skip, so events may be dropped on it early
            assert d == 0
        else:
            assert d >= 8, (v, d)


def test_the_wave_walk_and_its_monoid_equal_the_literal_loop():
    """what k_manifold_cells relies on: for events with 0 <= pz <= 65534 the per-event state functions compose as the monoid (T, M) under any
    bracketing, and the trip form (prefix minimum + one vote, literal walk for a trip with a wrapped height) is the loop"""
    rng = np.random.default_rng(17)
    starts = np.array([30000, 65535, 65534, 0, 9000, 65436, 12000])
    for it in range(4000):
        n = int(rng.integers(1, 40))
        pz = rng.integers(0, 65535, n) if it % 3 == 0 else rng.integers(8990, 9012, n)
        bad = rng.random(n) < (0.5 if it % 2 else 0.1)
        s0 = int(rng.choice(starts)) if it % 5 else int(rng.integers(0, 65536))
        want = M.walk_literal(s0, pz, bad)
        fs = [M.monoid_of(p, b) for p, b in zip(pz, bad)]
        while len(fs) > 1:                       # a random bracketing: neighbours merged in random order
            k = int(rng.integers(0, len(fs) - 1))
            fs[k:k + 2] = [M.monoid_compose(fs[k], fs[k + 1])]
        assert M.monoid_apply(fs[0], s0) == want, (s0, pz, bad)
        assert M.walk_trips(s0, pz, bad, width=int(rng.choice([1, 3, 8, 64]))) == want, (s0, pz, bad)
    for it in range(2000):                       # with wrapped heights: below 0, 65535 itself and above
        n = int(rng.integers(1, 200))
        pz = rng.integers(8990, 9012, n)
        wild = rng.random(n) < 0.05
        pz[wild] = rng.choice(np.array([-1, -100, -70000, 65535, 70000, 30001]), int(wild.sum()))
        bad = rng.random(n) < 0.2
        s0 = int(rng.choice(starts))
        assert M.walk_trips(s0, pz, bad, width=int(rng.choice([4, 64]))) == M.walk_literal(s0, pz, bad), (s0, pz, bad)
    # and on every cell's run of the injected case, where the crowd spans 82 trips
    case, rows = M.injected()
    ev = [M.events(P, N, case["resolution"], case["xs"], case["ys"]) for P, N in rows]
    x, y, inside, pz, normal, bad = [np.concatenate(v) for v in zip(*ev)]
    keep = inside & normal
    cell, pz, bad = (x * case["ys"] + y)[keep], pz[keep], bad[keep]
    perm = np.argsort(cell, kind="stable")
    cell, pz, bad = cell[perm], pz[perm], bad[perm]
    img = np.full(case["xs"] * case["ys"], M.UNTOUCHED, np.int64)
    cuts = np.nonzero(np.r_[True, cell[1:] != cell[:-1], True])[0]
    for a, b in zip(cuts[:-1], cuts[1:]):
        img[cell[a]] = M.walk_trips(M.UNTOUCHED, pz[a:b], bad[a:b])
    assert np.array_equal(img.reshape(case["xs"], case["ys"]).astype(np.uint16), M.splat(rows, case["resolution"], case["xs"], case["ys"])[0])


# ---------------------------------------------------------------------------------------------------------------- the mirrors
def test_mirror_names_and_defaults():
    from g2o_frontend_amd import api
    e = api.ManifoldVoronoiExtractor(cache=None)
    assert (e.xSize, e.ySize, e.normalThreshold, e.resolution(), e.dequeSize()) == (100, 100, 0.64, 0.2, 30)
    e.setQueueSize(3); e.setResolution(0.05)
    assert (e.dequeSize(), e.resolution()) == (3, 0.05)
    d = api.ManifoldVoronoiData()
    assert d.resolution == 0.2 and d.node is None and d.image is None
    hpp = open(os.path.join(ROOT, "g2o_frontend_amd", "host", "pwn_hip.hpp")).read()
    for text in ("class ManifoldVoronoiExtractor", "struct ManifoldVoronoiData", "setQueueSize", "dequeSize()", "setResolution", "int xSize = 100, ySize = 100",
                 "float normalThreshold = 0.64f", "float _resolution = 0.2f", "size_t _dequeSize = 30", "ManifoldVoronoiData process(const MapNode* keyNode)"):
        assert text in hpp, text
    # the transform is the merger's: inverse * transform in double, cast to float
    rng = np.random.default_rng(3)
    from test_merged_partition_cpu import pose
    A, B = (pose(int(rng.integers(3)), rng.uniform(-170, 170), rng.normal(size=3)) for _ in range(2))
    got = api.ManifoldVoronoiExtractor.nodeTransform(api.MapNode("a", A), api.MapNode("b", B))
    assert got.dtype == np.float32 and np.allclose(got, M.relative_transforms([A, B], 0)[1], rtol=0, atol=1e-6)


def test_new_entry_point_is_declared_prototyped_and_refuses_null_arguments_without_a_device():
    from g2o_frontend_amd import _lib
    assert len(_lib.PROTOTYPES["pwn_hip_manifold_image"][1]) == 11
    header = open(os.path.join(ROOT, "include", "pwn_hip.h")).read()
    assert "int pwn_hip_manifold_image(" in header and "manifold_voronoi_extractor.cpp:50-127" in header and "undefined in the reference" in header
    L = _lib.lib()
    assert L.pwn_hip_manifold_image(None, 0, None, None, 0.2, 100, 100, 0.64, 0, None, None) == 1
    assert L.pwn_hip_last_error_string(None)
