"""The injected scene clouds on the CPU (tests/scene_clouds.py): the generators' own assertions, the oracle against the models -- the collapsed
indices of Merger::merge equal the construction, the survivors of VoxelCalculator::compute and their order equal the numpy model, the
Gaussian setter round-trips bit for bit -- and the oracle's fused means and transformed moments against float64 within the measured bars
(docs/parity.md, "Injected scene clouds")."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_clouds as S      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def side(oracle):
    return S.OracleSide(oracle)


# ------------------------------------------------------------------------------------------------------------------ the setter
def test_oracle_setter_round_trips(oracle):
    src = S.add_source()
    for ng in (0, 1, src["n"] - 3, src["n"]):
        c = S.oracle_cloud(oracle, src["arrays"], S.head_gauss(src["gauss"], ng))
        assert c.num_gaussians() == ng and len(c) == src["n"]
        got = c.gaussians()
        for k in S.GAUSS_KEYS:
            assert got[k].tobytes() == S.head_gauss(src["gauss"], ng)[k].tobytes(), (ng, k)
    g = S.cat_gauss(src["gauss"], S.tail_gaussians(9, src["n"]))            # more records than points
    c = S.oracle_cloud(oracle, src["arrays"], g)
    assert c.num_gaussians() == src["n"] + 9 and c.gaussians()["mean"].tobytes() == g["mean"].tobytes()
    bad = dict(g, flags=np.full(len(g["flags"]), 4, np.int32))
    with pytest.raises(ValueError):
        c.set_gaussian_arrays(*[bad[k] for k in S.GAUSS_KEYS])
    assert c.gaussians()["flags"].tobytes() == g["flags"].tobytes()         # a refusal writes nothing
    assert set(np.unique(src["gauss"]["flags"])) == {1, 2, 3}
    g = src["gauss"]
    assert (g["mean"][(g["flags"] & 1) == 0] == S.FILL_MOMENTS).all() and (g["info"][(g["flags"] & 2) == 0] == S.FILL_INFO).all()
    assert np.abs(g["mean"][(g["flags"] & 1) != 0] - src["arrays"]["points"][(g["flags"] & 1) != 0, :3]).max() > 1e-3      # means are not the points


# --------------------------------------------------------------------------------------------------------------- Merger::merge
@pytest.mark.parametrize("name", [n for n, _ in S.merge_cases()])
def test_oracle_collapsed_indices_equal_the_construction(oracle, name):
    case = dict(S.merge_cases())[name]
    S.check_placement(oracle, case["arrays"]["points"], case["r"], case["c"])
    c = S.oracle_cloud(oracle, case["arrays"], case["gauss"])
    k, col = S.oracle_merge(oracle, c, case["cfg"])
    assert np.array_equal(col, case["expect"])
    idx = np.arange(case["n"])
    keep = (col < 0) | (col == idx)
    assert k == keep.sum() == len(c) and c.num_gaussians() == case["n"]
    after = c.arrays()
    assert np.array_equal(after["normals"].view(np.uint32), case["arrays"]["normals"][keep].view(np.uint32))
    untouched = col[keep] < 0
    assert np.array_equal(after["points"][untouched], case["arrays"]["points"][keep][untouched])
    err = S.fused_error(after["points"], case["gauss"], col)
    print("%s: worst relative error of the fused means %.3g (bar %.0e)" % (name, err, S.fused_bar(name)))
    assert err <= S.fused_bar(name)
    # a winner without members moves too: to its Gaussian's mean, which is not where the point was
    alone = np.nonzero((col == idx) & ~np.isin(idx, col[(col >= 0) & (col != idx)]))[0]
    if len(alone):
        pos = np.cumsum(keep) - 1
        moved = np.abs(after["points"][pos[alone], :3] - case["arrays"]["points"][alone, :3]).max(1)
        assert (moved > 1e-4).mean() > 0.9


def test_oracle_merge_of_ill_conditioned_gaussians(oracle):
    """condition number 1e6: the decisions are the construction's; the fused means are held against nothing here (float32 inverses of such
    matrices carry no digits worth a bar) -- the device must still equal the oracle in every bit (tests/test_gpu_scene_clouds.py)"""
    case = S.flags_case(seed=17, cond=1e6)
    c = S.oracle_cloud(oracle, case["arrays"], case["gauss"])
    k, col = S.oracle_merge(oracle, c, case["cfg"])
    assert np.array_equal(col, case["expect"]) and k == ((col < 0) | (col == np.arange(case["n"]))).sum()
    C = case["gauss"]["cov"][(case["flags"] & 1) != 0].astype(np.float64).reshape(-1, 3, 3)
    assert np.linalg.cond(C).max() > 5e5


def test_merge_coverage_counts():
    thr = S.thresholds_case(False)["cover"]; far = S.thresholds_case(True)["cover"]
    for f in ("dist", "dot", "min", "maxdepth"):
        assert thr[f + "/below"] >= 8 and thr[f + "/above"] >= 8 and thr[f + "/equal"] >= 1
    assert far["max/below"] >= 8 and far["max/above"] >= 8 and far["max/equal"] >= 1
    lists = S.lists_case()
    lengths = {L: int((lists["tag"] == "list%d/member" % L).sum()) for L in S.LIST_LENGTHS}
    assert lengths == {L: L for L in S.LIST_LENGTHS}
    fl = S.flags_case()
    combos = {(ft, fm) for ft in (1, 2, 3) for fm in (1, 2, 3) if (fl["tag"] == "t%d/m%d/member" % (ft, fm)).sum() >= 2}
    assert len(combos) == 9
    print("thresholds:", thr, far, "lists:", lengths)


def test_oracle_merge_keeps_the_gaussian_tail_and_merges_again(oracle):
    """n_gauss > n: after each of two merges (the second under another pose) the whole Gaussian vector -- the compacted head, the members'
    cached information forms behind it, the tail -- is what the construction says"""
    case = S.flags_case(tail=37)
    n = case["n"]
    c = S.oracle_cloud(oracle, case["arrays"], case["gauss"])
    k, col = S.oracle_merge(oracle, c, case["cfg"])
    assert np.array_equal(col, case["expect"]) and c.num_gaussians() == n + 37
    g0, g1 = case["gauss"], c.gaussians()
    keep = np.nonzero((col < 0) | (col == np.arange(n)))[0]
    assert np.array_equal(g1["mean"][n:], g0["mean"][n:]) and np.array_equal(g1["flags"][n:], g0["flags"][n:])     # the tail
    members = np.nonzero((col >= 0) & (col != np.arange(n)))[0]
    stale = members[members >= k]                                             # entries the compaction did not overwrite
    assert len(stale) and ((g1["flags"][stale] & 2) != 0).all()              # addInformation cached their information form there
    had = stale[(g0["flags"][stale] & 2) != 0]
    assert np.array_equal(g1["info"][had], g0["info"][had])
    for t in np.nonzero(col == np.arange(n))[0]:
        j = int(np.searchsorted(keep, t))
        has_members = (col == t).sum() > 1
        assert g1["flags"][j] == (3 if has_members or g0["flags"][t] == 3 else (g0["flags"][t] | 1))
    k2, col2 = S.oracle_merge(oracle, c, case["cfg"], S.isometry((0.02, -0.01, 0.0, 0.0, 0.03, 0.0)))
    assert k2 <= k and c.num_gaussians() == n + 37 and np.array_equal(c.gaussians()["mean"][n:], g0["mean"][n:])


# ------------------------------------------------------------------------------------------------------------------ Cloud::add
@pytest.mark.parametrize("source", ["uploaded", "added", "converted"])
@pytest.mark.parametrize("dst_kind", S.ADD_DESTINATIONS)
def test_oracle_add_against_float64(side, source, dst_kind):
    src = S.add_source()
    worst = [0.0, 0.0]
    for tname, T in S.ADD_TRANSFORMS:
        for ngauss in (0, src["n"] - 3, src["n"]):
            (after_add, after_tr), g, gd, n = S.add_sequence(side, ngauss, dst_kind, T, source)
            k = 0 if dst_kind == "empty" else 70
            ng = 0 if g is None else len(g["flags"])
            assert len(after_add["points"]) == k + n
            # cloud.cpp:153 resizes to k + the source's count whatever either side holds: k default records when neither has Gaussians
            want_ng = k + ng
            assert len(after_add["gauss"]["flags"]) == want_ng, (tname, ngauss)
            ga = after_add["gauss"]
            if gd is not None:                                                # the destination's own records stay as they were
                for key in S.GAUSS_KEYS:
                    assert ga[key][:k].tobytes() == gd[key].tobytes()
            elif want_ng:
                assert (ga["flags"][:k] == 0).all()                           # default Gaussians for the points it held
            if g is None:
                continue
            if tname == "identity":                                           # cloud.cpp:176: nothing is touched, the information forms included
                for key in S.GAUSS_KEYS:
                    assert ga[key][k:].tobytes() == g[key].tobytes()
            else:
                assert (ga["flags"][k:] == 1).all() and (ga["info"][k:] == 0).all()
                em, ec = S.added_error(S.head_gauss({q: v[k:] for q, v in ga.items()}, ng), g, T)
                worst = [max(worst[0], em), max(worst[1], ec)]
            # transformInPlace on the result: every record with a valid form moves once more
            gt = after_tr["gauss"]
            sel = ga["flags"] != 0
            em, ec = S.added_error({q: v[sel] for q, v in gt.items()}, {q: v[sel] for q, v in ga.items()}, S.T_B)
            worst = [max(worst[0], em), max(worst[1], ec)]
            assert (gt["flags"][sel] == 1).all()
    print("%s -> %s: worst relative error of transformed means %.3g (bar %.0e), covariances %.3g (bar %.0e)"
          % (source, dst_kind, worst[0], S.BAR_ADD_MEAN, worst[1], S.BAR_ADD_COV))
    assert worst[0] <= S.BAR_ADD_MEAN and worst[1] <= S.BAR_ADD_COV


@pytest.mark.parametrize("dst_kind", S.ADD_DESTINATIONS)
def test_oracle_add_of_more_gaussians_than_points(side, dst_kind):
    for tname, T in S.ADD_TRANSFORMS:
        (a, t), k, n = S.add_long_sequence(side, dst_kind, T)
        ga = a["gauss"]
        assert len(a["points"]) == k + n and len(ga["flags"]) == k + n + S.LONG_TAIL
        assert (ga["flags"][k + n:] == 0).all() and (ga["cov"][k + n:] == 0).all() and (ga["flags"][k:k + n] != 0).all()
        assert (ga["flags"][:k] == 0).all() or dst_kind == "gaussians"
        assert (t["gauss"]["flags"] == 1).all()                               # transformInPlace declares every record's moments valid


# --------------------------------------------------------------------------------------------------------- VoxelCalculator
@pytest.mark.parametrize("name", [n for n, _ in S.voxel_cases()])
def test_oracle_voxel_grid_equals_the_numpy_model(oracle, name):
    case = dict(S.voxel_cases())[name]
    c = S.oracle_cloud(oracle, case["arrays"])
    k, kept = oracle.voxelize(c, case["res"], literal=False)
    assert k == len(case["kept"]) and np.array_equal(kept, case["kept"])
    a = c.arrays()
    for key in S.CLOUD_KEYS:
        assert np.array_equal(a[key].view(np.uint32), case["arrays"][key][case["kept"]].view(np.uint32)), key
    keys = case["keys"][kept]
    assert (np.diff(S.pack_keys(keys).astype(np.int64)) > 0).all()              # strictly ascending words = lexicographic order


def test_voxel_generators_cover_what_they_claim():
    d = S.voxel_digits_case()
    assert min(d["digit_values"]) >= 40 and np.abs(d["keys"]).max() > (1 << 20) - 5000
    g = S.voxel_stability_case()["groups"]                                    # pass -> (size, 64-record steps, chunks of 2048) on entering the pass
    assert g[2] == (3, 1, 1) and g[5][0] == 65 and g[5][1] >= 30 and g[5][2] == 1 and g[7][0] == 300 and g[7][1] >= 30 and g[7][2] == 2
    assert min(S.voxel_probe_case()["planted"]) >= 6
    for m in S.VOXEL_SURVIVORS:
        assert len(S.voxel_survivors_case(m, True)["kept"]) == m and S.voxel_survivors_case(m, True)["n"] > m
    for n in S.VOXEL_SIZES:
        e = S.voxel_sizes_case(n, "edges")
        for edge in (255, 511, 767, 1023):
            if edge < n - 1:
                assert edge in e["kept"] and (e["keys"][edge + 1] == e["keys"][edge]).all()


def test_oracle_voxel_bound_and_gaussian_rule(oracle):
    for axis, sign, case, bad in S.voxel_bound_cases():
        c = S.oracle_cloud(oracle, case["arrays"])
        k, kept = oracle.voxelize(c, case["res"], literal=False)
        assert np.array_equal(kept, case["kept"]) and kept[-1 if sign > 0 else 0] == 17
        assert abs(float(bad["points"][17, axis]) / case["res"]) == 2.0 ** 20
    case = S.voxel_survivors_case(65, True)
    n = case["n"]
    g = S.gaussians(np.random.default_rng(3), case["arrays"]["points"], 1 + np.arange(n) % 3)
    for ng in (n, n - 1, n + 1):
        gg = S.head_gauss(S.cat_gauss(g, S.tail_gaussians(1, n)), ng)
        c = S.oracle_cloud(oracle, case["arrays"], gg)
        k, kept = oracle.voxelize(c, case["res"], literal=False)
        got = c.gaussians()
        if ng == n:                                                           # voxelcalculator.cpp:62-64
            for key in S.GAUSS_KEYS:
                assert got[key].tobytes() == g[key][kept].tobytes()
        else:
            assert c.num_gaussians() == 0


def test_oracle_voxel_carry_case(oracle):
    """1024 * 1024 + 1025 points (a scan of more than 1024 block sums).  The slow case of this file: about 10 s, numpy's row-wise unique and
    the oracle's std::map; no marker for slow tests is registered, so it carries none (docs/parity.md)"""
    case = S.voxel_carry_case()
    c = S.oracle_cloud(oracle, case["arrays"])
    k, kept = oracle.voxelize(c, case["res"], literal=False)
    assert k == len(case["kept"]) and np.array_equal(kept, case["kept"])
    assert np.array_equal(c.arrays()["points"], case["arrays"]["points"][case["kept"]])
    S.voxel_carry_case.cache_clear()


# ------------------------------------------------------------------------------------------- the stand-alone sanitizer program
def test_setter_check_program_runs_clean_under_the_sanitizers():
    """oracle/set_gaussians_check.cpp with the oracle's source as one program of its own (nothing of it is loaded into Python), built by
    `make -C oracle set_gaussians_check_asan` with AddressSanitizer and UBSan -- only when a source is newer than the program -- and run"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "set_gaussians_check_asan"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "oracle", "set_gaussians_check_asan")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
