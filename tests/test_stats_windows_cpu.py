"""CPU twin of tests/test_gpu_stats_windows.py: the adversarial stats windows of tests/stats_windows.py through the oracle
(orc_stats_from_integral), checked against plain float64 with no GPU involved.  It sets the float64 bars (stats_windows.EIG_BARS) the GPU
test uses, and prints the measured worst values next to them."""
import numpy as np

import stats_windows as W


def test_oracle_split_keeps_convert_bits(oracle):
    """orc_stats_from_integral on the oracle's own integral image of a frame gives what orc_convert gives"""
    from conftest import case_params, make_depth_pair
    rows, cols, K, conv, _ = case_params("small")
    depth, _, _, _, _ = make_depth_pair("small", 3)
    p = oracle.converter_params(K=K, **conv)
    c, idx, itv = oracle.convert(p, depth)
    a = c.arrays(stats=True)
    pts, idx2 = oracle.unproject(p, depth)
    assert np.array_equal(idx, idx2)
    b = oracle.stats_from_integral(p, oracle.integral_image(idx, pts), idx, itv, pts).arrays(stats=True)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_stats_windows_oracle_against_float64(oracle):
    frames = W.make_frames(11, 480, 640, 3, ["A", "B", "R"]) + W.make_frames(12, 97, 300, 2, ["A", "A"])
    outs = [W.run_oracle(oracle, W.converter_params(oracle), f) for f in frames]
    reps = [W.check_against_float64([f], [o], W.CONV) for f, o in zip(frames, outs)]
    win, worst = {}, {}
    for r in reps:
        for k, v in r["windows"].items():
            win[k] = win.get(k, 0) + v
        for k, v in r["worst_eig"].items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k in sorted(win):
        print(f"  {k:15s} {win[k]:8d} windows, worst |d lambda| / lambda_max {worst[k]:.2e} (bar {W.EIG_BARS[k]:.1e})")
    print(f"  worst normal angle / bar {max(r['worst_normal'] for r in reps):.2f}; decisions within the bar of a threshold that differ from "
          f"float64: {sum(r['near_threshold'] for r in reps)}")
    for k in W.FAMILIES:
        if k not in ("idx_neg", "itv_neg"):
            assert win.get(k, 0) >= 100, k


# ------------------------------------------------------------------------------------------------ the lean frames' generator, held to its claims
import pytest


@pytest.fixture(scope="module")
def lean_sets(oracle):
    """the frames of every lean setting with the oracle's results, made once"""
    out = []
    for k, (rows, cols, nf, layouts, omega, offset, raw, _) in enumerate(W.LEAN_SETTINGS):
        frames = W.make_lean_frames(oracle, 300 + k, rows, cols, nf, layouts, raw, offset)
        p = W.lean_params(oracle, offset)
        out.append((frames, [W.run_oracle(oracle, p, f) for f in frames], p))
    return out


def test_lean_camera_is_what_the_generator_restates(oracle):
    """LEAN_IV and lean_quotient restate the oracle's projectInterval for the lean camera: int(quotient) is the oracle's interval on depths of
    every magnitude and both signs"""
    rng = np.random.default_rng(1)
    d = (rng.uniform(0.01, 300, (40, 50)) * np.sign(rng.standard_normal((40, 50)))).astype(np.float32)
    itv = oracle.project_intervals(W.lean_params(oracle), d)
    assert np.array_equal(itv, W.lean_quotient(d).astype(np.int32))
    assert np.float32(W.LEAN_IV) == np.float32(512.0) * np.float32(0.01)


def test_lean_layout_a_depths_give_the_intervals_the_layout_needs(lean_sets, oracle):
    """Layout A: every probe's oracle interval is 0 or 1 (radius 1 after the clamp), negative on the itv_neg probes of float frames, and raw
    frames express every depth (the oracle's conversion of the uint16 image is the depth both sides see)"""
    seen = {"0": 0, "1": 0, "neg": 0}
    for (rows, cols, nf, layouts, omega, offset, raw, _), (frames, outs, p) in zip(W.LEAN_SETTINGS, lean_sets):
        for fr in frames:
            if raw:
                assert fr.raw.dtype == np.uint16 and np.array_equal(oracle.convert_16u_to_32f(fr.raw, W.LEAN_RAW_SCALE).view(np.uint32), fr.depth.view(np.uint32))
            else:
                assert fr.raw is None and fr.depth.dtype == np.float32
            assert np.array_equal(fr.interval, oracle.project_intervals(p, fr.depth))
            if not W.is_layout_a(fr):
                continue
            has = (fr.index >= 0) & ~fr.undefined
            fam = np.full(fr.index.shape, "", object); fam[fr.index >= 0] = fr.family[fr.index[fr.index >= 0]]
            neg = has & (fam == "itv_neg")
            assert np.isin(fr.interval[has & ~neg], (0, 1)).all()
            assert (fr.interval[neg] < 0).all() and (fr.depth[neg] < 0).all()
            assert raw or neg.sum() == (fam == "itv_neg").sum() > 0
            seen["0"] += int((fr.interval[has] == 0).sum()); seen["1"] += int((fr.interval[has] == 1).sum()); seen["neg"] += int(neg.sum())
    print("layout A, oracle intervals under points:", seen)
    assert seen["0"] > 1000 and seen["1"] > 1000 and seen["neg"] >= 4 * W.MIN_BRANCH


def test_lean_flip_zero_column_and_undefined_conversions(lean_sets, oracle):
    """flip_zero is one probe column in which the oracle's unprojected x is exactly zero; its depths are positive, +0 and (float) -0.0.  A zero
    depth makes an infinite quotient: the mask of undefined conversions is exactly what the generator placed (these probes, and the itv_neg
    probes of raw frames), in every frame, and holds nothing in the dense layouts.  What the oracle returns there is printed."""
    kinds, at_zero = {"positive": 0, "+0": 0, "-0": 0}, {}
    for (rows, cols, nf, layouts, omega, offset, raw, _), (frames, outs, p) in zip(W.LEAN_SETTINGS, lean_sets):
        for fr in frames:
            assert np.array_equal(fr.undefined, fr.placed_undefined & (fr.index >= 0)) and np.array_equal(fr.undefined, fr.placed_undefined)
            q = W.lean_quotient(fr.depth)
            assert np.array_equal(fr.undefined, (fr.index >= 0) & ~np.isfinite(q)) and (np.abs(q[(fr.index >= 0) & ~fr.undefined]) < 2.0 ** 31).all()
            if not W.is_layout_a(fr):
                assert not fr.undefined.any()
                continue
            fz = fr.family == "flip_zero"
            rr, cc = np.nonzero(fr.index >= 0)
            col = np.zeros(len(fr.points), np.int64); col[fr.index[rr, cc]] = cc
            dep = np.zeros(len(fr.points), np.float32); dep[fr.index[rr, cc]] = fr.depth[rr, cc]
            assert (col[fz] == W.LEAN_FLIP_COL).all() and fz.sum() == (col == W.LEAN_FLIP_COL).sum() == len(range(2, rows, 3))
            assert (fr.points[fz, 0] == 0).all(), "the oracle's unprojected x is not exactly zero in the flip_zero column"
            und = W.undefined_points(fr)
            assert (fr.points[~fz & ~und, 0] != 0).all()
            kinds["positive"] += int((dep[fz] > 0).sum())
            kinds["+0"] += int(((dep[fz] == 0) & ~np.signbit(dep[fz])).sum()); kinds["-0"] += int(((dep[fz] == 0) & np.signbit(dep[fz])).sum())
            assert ((dep[fz] > 0) | (dep[fz] == 0)).all()
            assert np.array_equal(und[fz], dep[fz] == 0)
            assert raw or not und[~fz].any()
            assert not raw or np.array_equal(und & ~fz, fr.family == "itv_neg")
            for dv, iv in zip(fr.depth[fr.undefined], fr.interval[fr.undefined]):
                key = ("-0" if np.signbit(dv) else "+0", int(iv))
                at_zero[key] = at_zero.get(key, 0) + 1
    print("flip_zero depths:", kinds, "; oracle's interval at a zero depth (depth, interval): pixels", at_zero)
    assert min(kinds.values()) >= 50


def test_lean_dense_layouts_meet_both_clamps_and_the_skip_at_every_border(lean_sets):
    """B and R: under points the oracle's intervals run from below min_image_radius to above max_image_radius, float frames hold negative depths
    (the skip), and each of the four borders holds a point pixel below the lower clamp, above the upper clamp and (float) a skipped one"""
    n = 0
    for (rows, cols, nf, layouts, omega, offset, raw, _), (frames, outs, p) in zip(W.LEAN_SETTINGS, lean_sets):
        for fr in frames:
            if W.is_layout_a(fr):
                continue
            n += 1
            has = fr.index >= 0
            itv = fr.interval
            lo, hi = W.CONV["min_image_radius"], W.CONV["max_image_radius"]
            assert ((itv >= 0) & (itv < lo) & has).any() and ((itv > hi) & has).any() and ((itv >= lo) & (itv <= hi) & has).any()
            assert raw == (not ((fr.depth < 0) & has).any())
            for sel in (np.s_[0, :], np.s_[rows - 1, :], np.s_[:, 0], np.s_[:, cols - 1]):
                b, h = itv[sel], has[sel]
                assert ((b >= 0) & (b < lo) & h).any() and ((b > hi) & h).any(), sel
                assert raw or ((b < 0) & h).any(), sel
    assert n >= 8


def test_lean_generator_meets_the_coverage_floor_on_the_cpu(lean_sets, oracle):
    """MIN_BRANCH windows per entry of COVERED, summed over the layout-A frames of each setting, from the oracle's outputs: the generator alone
    meets what the GPU test asserts"""
    for setting, (frames, outs, p) in zip(W.LEAN_SETTINGS, lean_sets):
        if not any(W.is_layout_a(f) for f in frames):
            continue
        cover = {k: 0 for k in W.COVERED}
        for fr, o in zip(frames, outs):
            if W.is_layout_a(fr):
                for k, v in W.coverage(oracle, fr, o).items():
                    cover[k] += v
        print(f"setting {setting}: {cover}")
        for k in W.lean_covered(setting[6]):
            assert cover[k] >= W.MIN_BRANCH, (setting, k, cover[k])


def test_lean_frames_oracle_against_float64(lean_sets, oracle):
    """the oracle on lean frames (points and intervals derived from the depth) obeys the float64 bars the GPU test applies; the pixels of an
    undefined conversion are left out (the numpy model and the oracle need not agree on the window there)"""
    frames = W.make_lean_frames(oracle, 400, 97, 300, 3, ["A", "B", "R"], raw=False)
    p = W.lean_params(oracle)
    win = {}
    for fr in frames:
        f2, o2 = W.without_points(fr, W.run_oracle(oracle, p, fr), W.undefined_points(fr))
        for k, v in W.check_against_float64([f2], [o2], W.CONV)["windows"].items():
            win[k] = win.get(k, 0) + v
    assert win["dense"] > 10000 and win["dense_raw"] > 1000 and win["flip_zero"] >= 10
