"""The converter's stats pass (k_stats, the shipped kernel, through pwn_hip_debug_stats_from_integral) on adversarial windows
(tests/stats_windows.py): against the oracle bit for bit, against plain float64 with no oracle, and the eigensolver's trig on the device
against the oracle's canonical evaluation and mpmath."""
import numpy as np
import pytest

import stats_windows as W

pytestmark = pytest.mark.gpu

# (rows, cols, frames, layouts dealt round-robin, omega storage, sensor offset).  Every setting is ONE launch of k_stats over all its frames (the
# layouts share one parameter set): 1 and 7 frames take the frame-major placement, 8 and 13 the XCD-aware one (13: a partial last group of 8);
# both sizes, both storages, the dense layouts and the offset meet the XCD-aware placement.  ~3.6 M windows in all.
SETTINGS = [(480, 640, 1, ["B"], "exact9", False), (97, 300, 7, ["A", "B", "R"], "sym6", True),
            (480, 640, 8, ["A", "B"], "sym6", False), (480, 640, 13, ["A", "A", "R"], "exact9", True),
            (97, 300, 13, ["A", "R", "B"], "sym6", True)]
MIN_BRANCH = 50      # windows per eig3_direct branch / edge, per setting with layout-A frames
COVERED = ("isotropic", "double_root", "scale_zero", "q_clamped", "half_b_zero", "denormal_cov", "ev0_clamped", "near_threshold", "flip_zero",
           "n_below", "n_at", "n_above", "itv_neg", "idx_neg")


@pytest.fixture(scope="module")
def ctx():
    from g2o_frontend_amd import api
    c = api.Context(device=0, max_rows=480, max_cols=640, max_batch=13)
    yield c
    c.close()


def _is_a(fr):
    return fr.family.size == 0 or fr.family[0] not in ("dense", "dense_raw")


@pytest.mark.parametrize("setting", range(len(SETTINGS)))
def test_stats_windows_bit_exact_against_oracle(ctx, oracle, setting):
    rows, cols, nf, layouts, omega, offset = SETTINGS[setting]
    frames = W.make_frames(100 + setting, rows, cols, nf, layouts)
    p = W.converter_params(oracle, offset)
    outs, _ = W.run_gpu(ctx, p, frames, omega)                      # one pwn_hip_debug_stats_from_integral call: one k_stats launch of nf frames
    total, bad_all = 0, {}
    cover = {k: 0 for k in COVERED}
    for fr, g in zip(frames, outs):
        o = W.run_oracle(oracle, p, fr)
        bad = W.compare_to_oracle(o, g, sym6=(omega == "sym6"))
        for k, v in bad.items():
            bad_all[k] = bad_all.get(k, 0) + v
        total += fr.windows
        if _is_a(fr):
            n, has, mean, cov = W.window_cov(fr, W.CONV)
            br = W.eig_branches(oracle, cov[has])
            for k in ("isotropic", "double_root", "scale_zero", "q_clamped", "half_b_zero", "denormal_cov", "ev0_clamped"):
                cover[k] += int(br[k].sum())
            assert (g["eigenvalues"][has][br["ev0_clamped"], 0] == 0).all(), "a negative smallest eigenvalue was not clamped to 0"
            for key in W.THRESHOLDS:
                t = np.float32(W.CONV[key])
                cover["near_threshold"] += int((has & (np.abs(g["curvature"].view(np.int32) - t.view(np.int32)) <= 4)).sum())
            cover["flip_zero"] += int((has & (fr.family == "flip_zero") & (np.abs(g["normals"][:, :3]).sum(1) > 0)).sum())
            ne = fr.family == "n_edge"
            cnt = fr.planes[3][fr.index >= 0][np.argsort(fr.index[fr.index >= 0])]
            cover["n_below"] += int((ne & (cnt == 49)).sum()); cover["n_at"] += int((ne & (cnt == 50)).sum())
            cover["n_above"] += int((ne & (cnt == 51)).sum())
            cover["itv_neg"] += int(((fr.interval < 0) & (fr.index >= 0)).sum())
            cover["idx_neg"] += fr.windows - len(fr.points)
    print(f"setting {SETTINGS[setting]}: {total} windows in one launch; differing points per field {bad_all}")
    if any(_is_a(fr) for fr in frames):
        print(f"  branch / edge coverage: {cover}")
        for k in COVERED:
            assert cover[k] >= MIN_BRANCH, (k, cover[k])
    assert not any(bad_all.values()), bad_all


def test_stats_windows_against_float64(ctx, oracle):
    """no oracle in the comparison (it only builds the converter parameters): numpy fp32 sums / mean / covariance bit for bit, float64 LAPACK
    eigen-pairs within the per-family bars, what follows the eigen-solve bit for bit from the GPU's own eigen outputs"""
    frames = W.make_frames(200, 480, 640, 4, ["A", "A", "A", "A"]) + W.make_frames(201, 480, 640, 2, ["B", "R"])
    outs = W.run_gpu(ctx, W.converter_params(oracle), frames)[0]
    win, worst, wn, near = {}, {}, 0.0, 0
    for fr, g in zip(frames, outs):
        r = W.check_against_float64([fr], [g], W.CONV)
        for k, v in r["windows"].items():
            win[k] = win.get(k, 0) + v
        for k, v in r["worst_eig"].items():
            worst[k] = max(worst.get(k, 0.0), v)
        wn = max(wn, r["worst_normal"]); near += r["near_threshold"]
    for k in sorted(win):
        print(f"  {k:15s} {win[k]:8d} windows, worst |d lambda| / lambda_max {worst[k]:.2e} (bar {W.EIG_BARS[k]:.1e})")
    print(f"  worst normal angle / bar {wn:.2f}; decisions within the bar of a threshold that differ from float64: {near}")


def test_eigensolver_trig_on_device(ctx, oracle):
    """eig3_trig on the device against the oracle's canonical evaluation, bit for bit, over 16 M arguments: every binade the eigensolver
    produces (after its scaling the trace-free matrix has |S|_F^2 <= 9, so y = sqrt(q) and |half_b| stay below 2: binades down to the
    smallest denormal and up to [1, 2)), zeros of both signs, the axes, and arguments whose float64
    atan2 lies within 1e-12 of a float rounding boundary; for those, theta also against the one mpmath gives (correctly rounded atan2 times
    the float 1/3, at most 1 ulp)"""
    import mpmath
    rng = np.random.default_rng(5)
    n = 16 * 1024 * 1024
    e = rng.integers(-149, 2, (2, n)).astype(np.float64)          # random() * 2^e: every binade from the denormals to [1, 2)
    y = (rng.random(n) * 2.0 ** e[0]).astype(np.float32)
    x = ((rng.random(n) * 2 - 1) * 2.0 ** e[1]).astype(np.float32)
    y[:1000] = 0; x[:500] = np.float32(-0.0); x[500:1000] = 0.0; y[1000:2000] = 1.0; x[1000:1500] = 1.0; x[1500:2000] = -1.0
    x[2000:2500] = 0.0; x[2500:3000] = np.float32(-0.0); y[2000:3000] = rng.random(1000).astype(np.float32)
    # near a rounding boundary: float64 atan2 within 1e-12 (relative) of the midpoint of two floats
    a64 = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    af = a64.astype(np.float32)
    nb = np.nextafter(af, np.where(a64 > af, np.float32(np.inf), np.float32(-np.inf)))
    mid = (af.astype(np.float64) + nb.astype(np.float64)) / 2
    near = np.nonzero((np.abs(a64 - mid) <= 1e-12 * np.abs(a64)) & (a64 > 0))[0]
    g = W.trig_eval_gpu(ctx, y, x)
    o = oracle.trig_eval(0, y, x)
    for gv, ov, name in zip(g, o, ("theta", "cos", "sin")):
        same = gv.view(np.uint32) == ov.view(np.uint32)
        assert same.all(), f"{name}: {int((~same).sum())} of {n} differ from the oracle"
    assert np.all(g[0][:500] == np.float32(np.pi) * np.float32(1.0 / 3.0)) and np.all(g[0][500:1000] == 0)
    mpmath.mp.prec = 200
    off = 0
    for i in near:
        # the kernel rounds atan2 to float, then multiplies by the float 1/3: the same two steps from the correctly rounded atan2
        want = np.float32(float(mpmath.atan2(mpmath.mpf(float(y[i])), mpmath.mpf(float(x[i]))))) * np.float32(1.0 / 3.0)
        d = abs(int(g[0][i].view(np.int32)) - int(want.view(np.int32)))
        assert d <= 1, (float(y[i]), float(x[i]))
        off += d
    print(f"trig on the device: {n} arguments bit-identical to the oracle; {len(near)} near a rounding boundary, {off} of them 1 ulp off the "
          f"correctly rounded two-step value")
    assert len(near) >= 50 and off <= max(3, len(near) // 100)
