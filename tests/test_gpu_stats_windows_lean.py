"""The converter's stats pass as every lean convert call runs it (k_stats with cp.lean = kLeanGrouped, through
pwn_hip_debug_stats_from_integral_lean) on the adversarial windows of tests/stats_windows.py: the integral image in the grouped form -- four
16-byte loads of (x y z n), the decision n >= min_points, then the other eight loads -- and point and interval recomputed from a float or raw
depth frame.  Against the oracle bit for bit, the points included: the oracle's intervals and points are derived from the same depth
(stats_windows.lean_frame), never from the library.  Left out of a comparison: the pixels whose float-to-int conversion is undefined (a zero
depth under a point), exactly where the generator placed them (test_stats_windows_cpu.py)."""
import numpy as np
import pytest

import stats_windows as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts():
    """one context per slot size: exactly 97 x 300, exactly 61 x 257 (odd N: every second slot starts 8 bytes off a 16-byte boundary), and
    480 x 640 for the 97 x 300 call whose group bases lie inside a larger slot"""
    from g2o_frontend_amd import api
    made = {}

    def get(rows, cols, where):
        key = (480, 640) if where == "vga" else (rows, cols)
        if key not in made:
            made[key] = api.Context(device=0, max_rows=key[0], max_cols=key[1], max_batch=13)
        return made[key]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("setting", range(len(W.LEAN_SETTINGS)))
def test_lean_stats_windows_bit_exact_against_oracle(contexts, oracle, setting):
    rows, cols, nf, layouts, omega, offset, raw, where = W.LEAN_SETTINGS[setting]
    frames = W.make_lean_frames(oracle, 300 + setting, rows, cols, nf, layouts, raw, offset)
    p = W.lean_params(oracle, offset)
    outs, _ = W.run_gpu_lean(contexts(rows, cols, where), p, frames, omega)      # one call: one k_stats launch of nf frames
    total, masked, bad_all = 0, 0, {}
    cover = {k: 0 for k in W.COVERED}
    for fr, g in zip(frames, outs):
        assert np.array_equal(fr.undefined, fr.placed_undefined), "an undefined conversion the generator did not place"
        o = W.run_oracle(oracle, p, fr)
        und = W.undefined_points(fr)
        bad = W.compare_to_oracle(o, g, sym6=(omega == "sym6"), skip=und)
        for k, v in bad.items():
            bad_all[k] = bad_all.get(k, 0) + v
        total += fr.windows; masked += int(und.sum())
        if W.is_layout_a(fr):
            for k, v in W.coverage(oracle, fr, g).items():
                cover[k] += v
    print(f"setting {W.LEAN_SETTINGS[setting]}: {total} windows in one launch, {masked} of them undefined conversions (points compared, the rest "
          f"left out); differing points per field {bad_all}")
    if any(W.is_layout_a(fr) for fr in frames):
        print(f"  branch / edge coverage: {cover}")
        for k in W.lean_covered(raw):
            assert cover[k] >= W.MIN_BRANCH, (k, cover[k])
    assert not any(bad_all.values()), bad_all


def test_lean_stats_windows_against_float64(contexts, oracle):
    """no oracle in the comparison of the outputs (it builds the parameters and derives the frames' points and intervals from the depth): numpy
    fp32 sums / mean / covariance bit for bit, float64 LAPACK eigen-pairs within the existing per-family bars, what follows the eigen-solve bit
    for bit from the GPU's own eigen outputs -- four layout-A frames, one B and one R frame at 97 x 300, float depth, one launch"""
    frames = W.make_lean_frames(oracle, 500, 97, 300, 6, ["A", "A", "A", "A", "B", "R"], raw=False)
    outs = W.run_gpu_lean(contexts(97, 300, "own"), W.lean_params(oracle), frames)[0]
    win, worst, wn, near = {}, {}, 0.0, 0
    for fr, g in zip(frames, outs):
        f2, g2 = W.without_points(fr, g, W.undefined_points(fr))
        r = W.check_against_float64([f2], [g2], W.CONV)
        for k, v in r["windows"].items():
            win[k] = win.get(k, 0) + v
        for k, v in r["worst_eig"].items():
            worst[k] = max(worst.get(k, 0.0), v)
        wn = max(wn, r["worst_normal"]); near += r["near_threshold"]
    for k in sorted(win):
        print(f"  {k:15s} {win[k]:8d} windows, worst |d lambda| / lambda_max {worst[k]:.2e} (bar {W.EIG_BARS[k]:.1e})")
    print(f"  worst normal angle / bar {wn:.2f}; decisions within the bar of a threshold that differ from float64: {near}")
    assert {"dense", "dense_raw", "flip_zero", "n_edge", "combine"} <= set(win)


@pytest.mark.parametrize("raw", [False, True], ids=["float", "raw"])
def test_the_two_storage_forms_agree(contexts, oracle, raw):
    """the same planes, index images and oracle-derived intervals and points through the ten-plane hook (intervals and points uploaded) and
    through the grouped, lean hook (both recomputed from the depth): every array the same, bit for bit, the stats included, outside the pixels
    of an undefined conversion (there the uploaded interval is the oracle's and the recomputed one the device's)"""
    ctx = contexts(97, 300, "own")
    frames = W.make_lean_frames(oracle, 600 + int(raw), 97, 300, 9, ["A", "B", "R"], raw=raw, offset=True)
    p = W.lean_params(oracle, offset=True)
    planes_out = W.run_gpu(ctx, p, frames, "sym6")[0]
    lean_out = W.run_gpu_lean(ctx, p, frames, "sym6")[0]
    points, differing = 0, 0
    for fr, a, b in zip(frames, planes_out, lean_out):
        keep = ~W.undefined_points(fr)
        assert set(a) == set(b)
        assert np.array_equal(a["points"].view(np.uint32), b["points"].view(np.uint32)), "points"
        for k in a:
            same = np.array_equal(a[k][keep].view(np.uint32), b[k][keep].view(np.uint32))
            differing += 0 if same else 1
            assert same, k
        points += int(keep.sum())
    print(f"two forms, {'raw' if raw else 'float'} depth: {points} points of {len(frames)} frames, every array identical ({differing} differing)")
