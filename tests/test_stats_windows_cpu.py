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
