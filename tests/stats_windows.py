"""Adversarial windows for the converter's stats pass (StatsCalculatorIntegralImage::compute after the integral image): integral planes,
index and interval images that no depth frame produces, fed to the GPU's k_stats (pwn_hip_debug_stats_from_integral) and to the oracle
(orc_stats_from_integral).  A helper module of the tests, imported by test_gpu_stats_windows.py and test_stats_windows_cpu.py.

All layouts share one converter parameter set (CONV: radii 1..60), so that the frames of a setting go to k_stats in one launch.

Layout A, private corners: probes on a stride-3 grid at (3i + 2, 3j + 2) whose interval is 0 or 1, clamped to radius 1 by min_image_radius.  getRegion
(pointintegralimage.cpp:53-66) reads the window of a probe at (r, c) from A = (r, c), B = (r - 2, c - 2), C = (r, c - 2), D = (r - 2, c): four
pixels no other probe reads, so the corner values set the window's sums as ((A + B) - C) - D.  With B = C = D = 0, mean 0 and a power-of-two
count n >= min_points, 1/n is exact and the covariance the kernel computes is the injected second moments times 1/n bit for bit: any fp32
matrix reaches the eigensolver directly.  The "combine" family writes all four corners to test the combine order.

Dense layouts: "B" the 2-D float32 prefix sums of random points, "R" raw random planes; windows at every pixel, radii 1..60 from the interval
image clamped at the image border, so corners are shared and clamped.

Lean frames (see "lean frames" below): the same layouts with a depth image under them, for the grouped, lean form of the pass
(pwn_hip_debug_stats_from_integral_lean): the interval image and the points are the oracle's, derived from that depth.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

F32 = np.float32
# distinct thresholds, so that each of the three is crossed on its own; defaults otherwise (min_points 50).  Radius 1..60: layout A's
# intervals (0 or 1) become radius 1, the dense layouts' (-3..79) are clamped to 60
CONV = dict(min_image_radius=1, max_image_radius=60, min_points=50, stats_curvature_threshold=0.2,
            point_info_curvature_threshold=0.02, normal_info_curvature_threshold=0.05)
THRESHOLDS = ("stats_curvature_threshold", "point_info_curvature_threshold", "normal_info_curvature_threshold")
# windows per family in one layout-A frame, as fractions of its probes (the rest: "distinct")
FAMILIES = dict(two_equal=0.08, three_equal=0.05, rank1=0.05, rank2=0.05, decades=0.10, denormal=0.04, zero=0.02, constant=0.03,
                far_off_centre=0.06, curvature=0.08, flip_zero=0.03, n_edge=0.06, itv_neg=0.02, idx_neg=0.02, combine=0.06)
SENSOR_OFFSET = np.array([[0.9950042, -0.0998334, 0.0, 0.05], [0.0998334, 0.9950042, 0.0, -0.02], [0.0, 0.0, 1.0, 0.1], [0, 0, 0, 1]],
                         np.float32)


def converter_params(O, offset=False):
    return O.converter_params(sensor_offset=SENSOR_OFFSET if offset else None, **CONV)


def random_rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def spectrum_cov(R, lam):
    """float64 R diag(lam) R^T rounded to float32 (n x 3 x 3)"""
    return np.einsum("nij,nj,nkj->nik", R, lam, R).astype(F32)


def sums_from_cov(cov, n):
    """window sums (x, y, z, n, xx, xy, xz, yy, yz, zz) with mean 0: the second moments n * cov (exact for a power-of-two n)"""
    s = np.zeros((len(cov), 10), F32)
    s[:, 3] = n
    nf = np.asarray(n, F32)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        s[:, 4 + k] = cov[:, i, j] * nf
    return s


def sums_from_points(P):
    """sums of a window's points accumulated in float32 one point after the other (m x k x 3 -> m x 10)"""
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    ch = [x, y, z, np.ones_like(x), x * x, x * y, x * z, y * y, y * z, z * z]
    out = np.zeros((P.shape[0], 10), F32)
    for k, v in enumerate(ch):
        acc = np.zeros(P.shape[0], F32)
        for t in range(P.shape[1]):
            acc = acc + v[:, t].astype(F32)
        out[:, k] = acc
    return out


def curvature_candidates(rng, m, thr):
    """diagonal covariances (in a random axis order) whose curvature lambda0 / (lambda0 + lambda1 + lambda2) lies around `thr`, lambda0 spread
    over a relative +-1e-4 around the exact ratio in log steps down to 1e-9: a few of them land within an ulp or two of the threshold"""
    l1 = 10.0 ** rng.uniform(-4, -1, m); l2 = l1 * rng.uniform(1.5, 4, m)
    d = np.sign(rng.standard_normal(m)) * 10.0 ** rng.uniform(-9, -4, m)
    l0 = thr / (1 - thr) * (l1 + l2) * (1 + d)
    lam = np.stack([l0, l1, l2], 1)
    perm = np.array([rng.permutation(3) for _ in range(m)])
    P = np.zeros((m, 3, 3)); P[np.arange(m)[:, None], perm, np.arange(3)[None, :]] = 1.0
    return spectrum_cov(P, lam)


class Frame:
    """One frame of windows: planes [10][rows][cols], index and interval images, the points the index image refers to, and a family label
    per output point"""

    def __init__(self, rows, cols):
        self.rows, self.cols = rows, cols
        self.planes = np.zeros((10, rows, cols), F32)
        self.index = np.full((rows, cols), -1, np.int32)
        self.interval = np.zeros((rows, cols), np.int32)
        self.points = np.zeros((0, 4), F32)
        self.family = np.zeros(0, object)
        self.windows = 0           # probes / pixels read by the stats pass (index >= 0 or not)


def layout_a(rng, rows, cols, thresholds=(0.2, 0.02, 0.05), flip_col=None):
    """flip_col: None = the flip_zero family is dealt like the others; a probe column = the family is exactly that column's probes (the lean
    frames, whose points come from the depth: one column where the unprojected x is zero)"""
    fr = Frame(rows, cols)
    ri, ci = np.arange(2, rows, 3), np.arange(2, cols, 3)
    R, Cc = np.meshgrid(ri, ci, indexing="ij")
    R, Cc = R.ravel(), Cc.ravel()
    m = len(R)
    fr.windows = m
    order = rng.permutation(m)
    fam = np.full(m, "distinct", object)
    if flip_col is not None:
        assert flip_col in ci
        fam[Cc == flip_col] = "flip_zero"
        order = order[Cc[order] != flip_col]
    start = 0
    for name, frac in FAMILIES.items():
        if flip_col is not None and name == "flip_zero":
            continue
        k = max(1, int(round(frac * m)))
        fam[order[start:start + k]] = name
        start += k
    sums = np.zeros((m, 10), F32)
    pts = (rng.standard_normal((m, 3)) * 2).astype(F32)
    pts[:, 2] = np.abs(pts[:, 2]) + 0.5
    pow2 = np.array([64, 128, 256, 1024], F32)

    def put(sel, cov, n=None):
        nn = rng.choice(pow2, len(sel)) if n is None else n
        sums[sel] = sums_from_cov(cov, nn)

    def spec(sel, lam, rotate=True):
        Rm = random_rotations(rng, len(sel)) if rotate else np.broadcast_to(np.eye(3), (len(sel), 3, 3))
        put(sel, spectrum_cov(Rm, lam))

    def idx(name):
        return np.nonzero(fam == name)[0]

    s = idx("distinct"); lam = np.sort(10.0 ** rng.uniform(-5, 0, (len(s), 3)), 1); spec(s, lam)
    s = idx("two_equal"); a = 10.0 ** rng.uniform(-5, 0, len(s)); b = a * 10.0 ** rng.uniform(-3, 1, len(s))
    lo = rng.random(len(s)) < 0.5
    spec(s, np.where(lo[:, None], np.stack([a, a, b], 1), np.stack([b, a, a], 1)))
    s = idx("three_equal"); a = 10.0 ** rng.uniform(-5, 1, len(s)); h = len(s) // 2
    spec(s[:h], np.stack([a[:h]] * 3, 1), rotate=False)              # exactly a * I: the isotropic branch
    spec(s[h:], np.stack([a[h:]] * 3, 1))                            # rotated: a * I up to the fp32 rounding of R diag R^T
    s = idx("rank1"); a = 10.0 ** rng.uniform(-4, 1, len(s)); z = np.zeros_like(a); spec(s, np.stack([z, z, a], 1))
    s = idx("rank2"); a = 10.0 ** rng.uniform(-4, 1, len(s)); b = a * rng.uniform(0.1, 1, len(s)); spec(s, np.stack([np.zeros_like(a), b, a], 1))
    s = idx("decades"); top = 10.0 ** rng.uniform(-28, 2, len(s))
    spec(s, top[:, None] * 10.0 ** -np.sort(rng.uniform(0, 30, (len(s), 3)), 1)[:, ::-1])
    s = idx("denormal"); top = 10.0 ** rng.uniform(-44, -36, len(s))    # the covariance itself below FLT_MIN (and for the smallest, n * cov too)
    spec(s, top[:, None] * 10.0 ** -np.sort(rng.uniform(0, 3, (len(s), 3)), 1)[:, ::-1])
    s = idx("zero"); put(s, np.zeros((len(s), 3, 3), F32))
    s = idx("constant")                                                 # every point equal: sums n p, n p p^T -> mean p, covariance 0
    p = (rng.standard_normal((len(s), 3)) * 3).astype(F32); n = rng.choice(pow2, len(s))
    sums[s, 0:3] = p * n[:, None]; sums[s, 3] = n
    for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        sums[s, 4 + k] = (p[:, i] * p[:, j]) * n
    s = idx("far_off_centre")                                           # 64 points ~1 mm around a centre ~10 m away, summed in fp32
    ctr = rng.standard_normal((len(s), 1, 3)) * 6
    P = (ctr + rng.standard_normal((len(s), 64, 3)) * 1e-3).astype(F32)
    sums[s] = sums_from_points(P)
    s = idx("curvature")                                                # curvature around each of the three thresholds
    for t, part in zip(thresholds, np.array_split(s, 3)):
        put(part, curvature_candidates(rng, len(part), t))
    s = idx("flip_zero")                                                # axis-aligned normal, point orthogonal to it (or zero, -0.0)
    lam = np.sort(10.0 ** rng.uniform(-4, 0, (len(s), 3)), 1); lam[:, 1:] *= 10
    spec(s, lam, rotate=False)                                          # normal = +-(1, 0, 0)
    pts[s, 0] = 0.0
    q = len(s) // 3
    pts[s[:q]] = 0.0
    pts[s[q:2 * q]] = F32(-0.0)
    s = idx("n_edge")                                                   # n = min_points - 1, min_points, min_points + 1 (1/n inexact)
    cov = spectrum_cov(random_rotations(rng, len(s)), np.sort(10.0 ** rng.uniform(-4, 0, (len(s), 3)), 1))
    sums[s] = sums_from_cov(cov, rng.choice(np.array([49, 50, 51], F32), len(s)))
    sums[s, 0:3] = rng.standard_normal((len(s), 3)).astype(F32) * sums[s, 3:4]
    for name in ("itv_neg", "idx_neg", "combine"):
        s = idx(name)
        cov = spectrum_cov(random_rotations(rng, len(s)), np.sort(10.0 ** rng.uniform(-4, 0, (len(s), 3)), 1))
        put(s, cov)
    # corners
    A = sums.copy()
    B = np.zeros_like(A); Cm = np.zeros_like(A); D = np.zeros_like(A)
    s = idx("combine")                                                  # large corners that cancel: the result depends on the order
    for X in (B, Cm, D):
        X[s] = (rng.standard_normal((len(s), 10)) * 1e3).astype(F32)
        X[s, 3] = rng.integers(0, 5000, len(s)).astype(F32)
    A[s] = ((sums[s] - B[s]) + Cm[s]) + D[s]
    A[s, 3] = sums[s, 3] - B[s, 3] + Cm[s, 3] + D[s, 3]               # integers: exact
    for X, dr, dc in ((A, 0, 0), (B, -2, -2), (Cm, 0, -2), (D, -2, 0)):
        fr.planes[:, R + dr, Cc + dc] = X.T
    itv = rng.integers(0, 2, m).astype(np.int32)                    # radius max(itv, min_image_radius) = 1
    itv[fam == "itv_neg"] = -rng.integers(1, 1000, (fam == "itv_neg").sum())
    fr.interval[R, Cc] = itv
    has_pt = fam != "idx_neg"
    fr.index[R[has_pt], Cc[has_pt]] = np.arange(has_pt.sum(), dtype=np.int32)
    fr.points = np.concatenate([pts[has_pt], np.ones((has_pt.sum(), 1), F32)], 1)
    fr.family = fam[has_pt]
    return fr


def layout_b(rng, rows, cols, raw=False):
    """dense windows: the integral image of random points (a 2-D float32 prefix sum, as the converter builds it), or (raw) random planes"""
    fr = Frame(rows, cols)
    fr.windows = rows * cols
    valid = rng.random((rows, cols)) < 0.92
    if raw:
        fr.planes[0:3] = (rng.standard_normal((3, rows, cols)) * 30).astype(F32)
        fr.planes[3] = rng.integers(0, 60, (rows, cols)).astype(F32)
        fr.planes[4:10] = (rng.standard_normal((6, rows, cols)) * 100).astype(F32)
        fr.planes[[4, 7, 9]] = np.abs(fr.planes[[4, 7, 9]]) * 3
    else:
        P = np.zeros((rows, cols, 3), F32)
        P[valid] = (rng.standard_normal((int(valid.sum()), 3)) * [0.3, 0.3, 0.05] + [0, 0, 2]).astype(F32)
        x, y, z = P[..., 0], P[..., 1], P[..., 2]
        for k, v in enumerate((x, y, z, valid.astype(F32), x * x, x * y, x * z, y * y, y * z, z * z)):
            fr.planes[k] = np.cumsum(np.cumsum(v, axis=1, dtype=F32), axis=0, dtype=F32)
    fr.interval = rng.integers(-3, 80, (rows, cols)).astype(np.int32)
    M = int(valid.sum())
    fr.index[valid] = rng.permutation(M).astype(np.int32)
    p = (rng.standard_normal((M, 3)) * 2).astype(F32)
    fr.points = np.concatenate([p, np.ones((M, 1), F32)], 1)
    fr.family = np.full(M, "dense_raw" if raw else "dense", object)
    return fr


def make_frames(seed, rows, cols, nframes, layouts):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(nframes):
        lay = layouts[i % len(layouts)]
        out.append(layout_a(rng, rows, cols) if lay == "A" else layout_b(rng, rows, cols, raw=(lay == "R")))
    return out


# ------------------------------------------------------------------------------------------------ lean frames
# A lean frame is a Frame plus a depth image: what k_stats sees behind the grouped front end, where neither points nor intervals are stored and
# the kernel recomputes both from the depth.  The interval image and the points of a lean frame are the ORACLE's, derived from that depth
# (lean_frame); the generator only chooses depths that make them what the layouts need.
#
# Camera and range.  fx = fy = 512 (a power of two) with the integer principal point (128, 47): in probe column 128 the unprojected x is
# (c d) / 512 - (128 / 512) d = 0 exactly (held to the oracle by the CPU test, not assumed).  world_radius 0.01 makes the interval int(5.12 / d):
# 0 beyond 5.12 m, 1 from 2.56 m, 79 at 64 mm -- all of it within uint16 millimetres.  k_stats does not repeat the front end's range test (a
# pixel with a point has passed it), so the range is opened to everything the generator injects, negative depths included: oracle and kernel
# then evaluate the same expression at every pixel, and what remains undefined is the float-to-int conversion of an infinite quotient
# (depth +0 / -0), which LeanFrame.undefined marks.
LEAN_K = (512.0, 512.0, 128.0, 47.0)
LEAN_FLIP_COL = 128
LEAN_CAMERA = dict(K=LEAN_K, world_radius=0.01, min_distance=-3.0e38, max_distance=3.0e38)
LEAN_RAW_SCALE = 0.001
LEAN_IV = 512.0 * float(F32(0.01))          # pixels of the world radius at unit depth, both axes (restated: the CPU test checks it with the oracle)


# (rows, cols, frames, layouts dealt round-robin, omega storage, sensor offset, raw depth, context).  Every setting is ONE launch.  97 x 300: an
# even N and two x-blocks per row; 61 x 257: an odd N, so that in a context of exactly 61 x 257 every second slot (40 N bytes each) starts 8 bytes
# off a 16-byte boundary; "vga": the 97 x 300 call runs in a 480 x 640 context, where the group bases 4 N and 8 N lie inside a larger slot.  1 and
# 7 frames take the frame-major placement, 8 and 13 the XCD-aware one (13: a ragged last group).  The frame counts of the layout-A frames are
# what the coverage floor needs at each shape (test_stats_windows_cpu.py holds the generator to it on the CPU).
LEAN_SETTINGS = [(97, 300, 1, ["B"], "exact9", False, False, "own"),
                 (97, 300, 7, ["A", "B", "A", "R", "A", "A", "A"], "sym6", True, False, "own"),
                 (61, 257, 8, ["A", "A", "A", "B", "A", "A", "R", "A"], "sym6", False, True, "own"),
                 (61, 257, 13, ["A", "A", "A", "B", "A", "A", "A", "R", "A", "A", "A", "A", "A"], "exact9", True, False, "own"),
                 (97, 300, 13, ["A", "R", "B", "A", "A", "A", "R", "A", "B", "A", "A", "A", "A"], "sym6", True, True, "vga"),
                 (97, 300, 8, ["A", "A", "B", "A", "R", "A", "A", "A"], "exact9", False, True, "own")]
MIN_BRANCH = 50      # windows per eig3_direct branch / edge, per setting with layout-A frames (test_gpu_stats_windows.MIN_BRANCH)
COVERED = ("isotropic", "double_root", "scale_zero", "q_clamped", "half_b_zero", "denormal_cov", "ev0_clamped", "near_threshold", "flip_zero",
           "n_below", "n_at", "n_above", "itv_neg", "idx_neg")


def lean_covered(raw):
    """the entries of COVERED a setting can meet: a raw frame has no negative depth, so its itv_neg probes hold raw 0 -- an undefined
    conversion, masked -- and the negative interval is left to the float settings"""
    return tuple(k for k in COVERED if not (raw and k == "itv_neg"))


def lean_params(O, offset=False):
    return O.converter_params(sensor_offset=SENSOR_OFFSET if offset else None, **dict(CONV, **LEAN_CAMERA))


def lean_quotient(depth):
    """projectInterval before its truncation, in numpy fp32: the larger of ivx * (1 / d) and ivy * (1 / d)"""
    iv = F32(512.0) * F32(0.01)
    with np.errstate(all="ignore"):
        inv = F32(1.0) / np.asarray(depth, F32)
        px, py = iv * inv, iv * inv
        return np.where(px > py, px, py).astype(F32)


def _depth_for_interval(rng, t, raw):
    """depths (metres, float64) whose interval int(iv / d) is t: t >= 1 -> iv / (t + u), u in [0.25, 0.75]; 0 -> beyond iv; t < 0 -> -iv / (|t| + u)"""
    t = np.asarray(t)
    u = rng.uniform(0.25, 0.75, t.shape)
    far = LEAN_IV * rng.uniform(1.05, 12.0 if raw else 40.0, t.shape)
    with np.errstate(divide="ignore"):
        return np.where(t > 0, LEAN_IV / (t + u), np.where(t == 0, far, -LEAN_IV / (np.abs(t) + u)))


def lean_frame(O, p, fr, rng, raw, dense):
    """Turns a Frame of layout_a(flip_col=LEAN_FLIP_COL) / layout_b into a lean one: chooses the depth image, then replaces fr.interval by
    oracle.project_intervals of it and fr.points by the oracle's per-pixel unprojection gathered by fr.index.  Adds fr.depth (float32 metres, as
    both implementations see it), fr.raw (the uint16 image, or None), fr.placed_undefined (where the generator put a zero depth under a point)
    and fr.undefined (where the quotient does not fit an int)."""
    rows, cols = fr.rows, fr.cols
    has = fr.index >= 0
    want = fr.interval.copy()                            # what the layout drew: 0 / 1 and negatives (A), -3 .. 79 (dense)
    placed = np.zeros((rows, cols), bool)
    if dense:
        if raw:
            want = np.abs(want)                          # uint16 holds no negative depth
        # both clamps and (float) the skip at all four borders, whatever the draw gave there
        for sel in (np.s_[0, :], np.s_[rows - 1, :], np.s_[:, 0], np.s_[:, cols - 1]):
            at = np.flatnonzero(has[sel])
            pick = rng.choice(at, 6, replace=False)
            want[sel][pick] = [0, 0, 70, 75, 2 if raw else -2, 3 if raw else -3]
        d = _depth_for_interval(rng, want, raw)
    else:
        d = _depth_for_interval(rng, np.where(has | (want != 0), want, rng.integers(0, 2, want.shape)), raw)
        fam_img = np.full((rows, cols), "", object)
        rr, cc = np.nonzero(has)
        fam_img[rr, cc] = fr.family[fr.index[rr, cc]]
        neg = has & (fam_img == "itv_neg")
        if raw:                                           # no negative raw value: these probes get raw 0, an undefined conversion
            d[neg] = 0.0; placed |= neg
        fz = np.flatnonzero((has & (fam_img == "flip_zero")).ravel())
        assert len(fz) and (fz % cols == LEAN_FLIP_COL).all()
        fz = rng.permutation(fz)
        k = max(1, len(fz) // 5)                          # a fifth +0, a fifth -0.0 (raw: +0 both), the rest positive
        d.ravel()[fz[:k]] = 0.0; d.ravel()[fz[k:2 * k]] = 0.0 if raw else -0.0
        placed.ravel()[fz[:2 * k]] = True
    if raw:
        counts = np.round(d / LEAN_RAW_SCALE)
        counts = np.where((counts < 1) & ~placed, 1, counts)              # raw 0 only where it was placed
        fr.raw = np.clip(counts, 0, 65535).astype(np.uint16)
        fr.depth = O.convert_16u_to_32f(fr.raw, LEAN_RAW_SCALE)
    else:
        fr.raw = None
        fr.depth = d.astype(F32)
    fr.placed_undefined = placed
    with np.errstate(invalid="ignore"):
        fr.undefined = has & ~(np.abs(lean_quotient(fr.depth)) < F32(2.0 ** 31))
    fr.interval = O.project_intervals(p, fr.depth)
    every, all_idx = O.unproject(p, fr.depth)            # the range is open: every pixel unprojects, point r * cols + c belongs to pixel (r, c)
    assert len(every) == rows * cols and np.array_equal(all_idx.ravel(), np.arange(rows * cols))
    pts = np.zeros((len(fr.points), 4), F32)
    pts[fr.index[has]] = every.reshape(rows, cols, 4)[has]
    fr.points = pts
    return fr


def make_lean_frames(O, seed, rows, cols, nframes, layouts, raw, offset=False):
    p = lean_params(O, offset)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(nframes):
        lay = layouts[i % len(layouts)]
        fr = layout_a(rng, rows, cols, flip_col=LEAN_FLIP_COL) if lay == "A" else layout_b(rng, rows, cols, raw=(lay == "R"))
        out.append(lean_frame(O, p, fr, rng, raw, dense=(lay != "A")))
    return out


def undefined_points(fr):
    """per point of the frame: its pixel's float-to-int conversion is undefined"""
    m = np.zeros(len(fr.points), bool)
    m[fr.index[fr.undefined]] = True
    return m


def without_points(fr, arrays, drop):
    """the frame and an implementation's arrays without the points `drop` marks (their pixels lose their index, the others are renumbered)"""
    keep = ~drop
    new = np.full(len(keep), -1, np.int32); new[keep] = np.arange(keep.sum(), dtype=np.int32)
    out = Frame(fr.rows, fr.cols)
    out.planes, out.interval, out.windows = fr.planes, fr.interval, fr.windows
    out.index = np.where(fr.index >= 0, new[np.maximum(fr.index, 0)], -1).astype(np.int32)
    out.points, out.family = fr.points[keep], fr.family[keep]
    return out, {k: v[keep] for k, v in arrays.items()}


def is_layout_a(fr):
    return fr.family.size == 0 or fr.family[0] not in ("dense", "dense_raw")


def coverage(O, fr, a, conv=CONV):
    """windows of a layout-A frame per eig3_direct branch / edge (test_gpu_stats_windows.COVERED), from the frame and one implementation's
    arrays `a`; pixels of an undefined conversion (lean frames) are not counted"""
    und = undefined_points(fr) if hasattr(fr, "undefined") else np.zeros(len(fr.points), bool)
    n, has, mean, cov = window_cov(fr, conv)
    has = has & ~und
    br = eig_branches(O, cov[has])
    cover = {k: int(br[k].sum()) for k in ("isotropic", "double_root", "scale_zero", "q_clamped", "half_b_zero", "denormal_cov", "ev0_clamped")}
    assert (a["eigenvalues"][has][br["ev0_clamped"], 0] == 0).all(), "a negative smallest eigenvalue was not clamped to 0"
    cover["near_threshold"] = 0
    for key in THRESHOLDS:
        t = F32(conv[key])
        cover["near_threshold"] += int((has & (np.abs(a["curvature"].view(np.int32) - t.view(np.int32)) <= 4)).sum())
    cover["flip_zero"] = int((has & (fr.family == "flip_zero") & (np.abs(a["normals"][:, :3]).sum(1) > 0)).sum())
    ne = (fr.family == "n_edge") & ~und
    cnt = fr.planes[3][fr.index >= 0][np.argsort(fr.index[fr.index >= 0])]
    for name, v in (("n_below", 49), ("n_at", 50), ("n_above", 51)):
        cover[name] = int((ne & (cnt == v)).sum())
    und_img = fr.undefined if hasattr(fr, "undefined") else np.zeros(fr.index.shape, bool)
    cover["itv_neg"] = int(((fr.interval < 0) & (fr.index >= 0) & ~und_img).sum())
    cover["idx_neg"] = fr.windows - len(fr.points)
    return cover


# ------------------------------------------------------------------------------------------------ the two implementations
def run_oracle(O, p, fr):
    c = O.stats_from_integral(p, fr.planes, fr.index, fr.interval, fr.points)
    return c.arrays(stats=True)


def run_gpu(ctx, p, frames, omega="exact9", keep_stats=True):
    """all frames in one call of the hook (one k_stats launch); the clouds read back as a convert call's"""
    from g2o_frontend_amd import api
    rows, cols = frames[0].rows, frames[0].cols
    ctx.set_omega_storage(omega)
    clouds = []
    for fr in frames:
        c = api.Cloud(ctx, max(1, len(fr.points)))
        n = len(fr.points)
        z4, z16 = np.zeros((n, 4), F32), np.zeros((n, 16), F32)
        c.upload(fr.points, z4, np.zeros(n, F32), z16, z16)
        clouds.append(c)
    planes = np.ascontiguousarray(np.stack([f.planes for f in frames]))
    idx = np.ascontiguousarray(np.stack([f.index for f in frames]))
    itv = np.ascontiguousarray(np.stack([f.interval for f in frames]))
    arr = (C.c_void_p * len(clouds))(*[c.h.value for c in clouds])
    ctx.check(ctx._L.pwn_hip_debug_stats_from_integral(ctx.h, C.addressof(p), rows, cols, len(frames), planes.ctypes.data_as(C.c_void_p),
                                                       idx.ctypes.data_as(C.c_void_p), itv.ctypes.data_as(C.c_void_p), arr, int(keep_stats)))
    return [c.arrays(stats=keep_stats) for c in clouds], clouds


def run_gpu_lean(ctx, p, frames, omega="exact9", keep_stats=True):
    """all lean frames in one call of pwn_hip_debug_stats_from_integral_lean (one k_stats launch with cp.lean = kLeanGrouped): the planes in the
    grouped form, the depth frames float or raw; the clouds give capacity only"""
    from depth_frames import planes_to_grouped
    from g2o_frontend_amd import api
    rows, cols = frames[0].rows, frames[0].cols
    raw = frames[0].raw is not None
    assert all((f.raw is not None) == raw for f in frames), "the frames of a call are all float or all raw"
    ctx.set_omega_storage(omega)
    clouds = [api.Cloud(ctx, max(1, len(fr.points))) for fr in frames]
    grouped = np.ascontiguousarray(np.stack([planes_to_grouped(f.planes) for f in frames]))
    idx = np.ascontiguousarray(np.stack([f.index for f in frames]))
    src = [np.ascontiguousarray(f.raw if raw else f.depth) for f in frames]
    assert src[0].dtype == (np.uint16 if raw else F32)
    arr = (C.c_void_p * len(clouds))(*[c.h.value for c in clouds])
    ptrs = (C.c_void_p * len(src))(*[a.ctypes.data for a in src])
    ctx.check(ctx._L.pwn_hip_debug_stats_from_integral_lean(ctx.h, C.addressof(p), rows, cols, len(frames), grouped.ctypes.data_as(C.c_void_p),
                                                            idx.ctypes.data_as(C.c_void_p), ptrs, LEAN_RAW_SCALE if raw else 0.0, arr, int(keep_stats)))
    for c, fr in zip(clouds, frames):
        assert c.size() == int(fr.index.max()) + 1 == len(fr.points)
    return [c.arrays(stats=keep_stats) for c in clouds], clouds


def trig_eval_gpu(ctx, y, x):
    y = np.ascontiguousarray(y, F32); x = np.ascontiguousarray(x, F32); n = y.size
    th, co, si = np.empty(n, F32), np.empty(n, F32), np.empty(n, F32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx.check(ctx._L.pwn_hip_debug_trig_eval(ctx.h, n, vp(y), vp(x), vp(th), vp(co), vp(si)))
    return th, co, si


# ------------------------------------------------------------------------------------------------ checks
def window_cov(fr, conv):
    """count, mean and covariance of every output point in numpy fp32, in the reference's order (pointintegralimage.cpp:61-64,
    pointaccumulator.h:66-86); returns (n, has, mean[m,3], cov[m,3,3]) per point of the frame (points without a window: has = False)"""
    rows, cols = fr.rows, fr.cols
    m = len(fr.points)
    rr, cc = np.nonzero(fr.index >= 0)
    pid = fr.index[rr, cc]
    itv = fr.interval[rr, cc]
    rad = np.clip(itv, conv["min_image_radius"], conv["max_image_radius"])
    xmin, xmax = np.clip(cc - rad - 1, 0, cols - 1), np.clip(cc + rad - 1, 0, cols - 1)
    ymin, ymax = np.clip(rr - rad - 1, 0, rows - 1), np.clip(rr + rad - 1, 0, rows - 1)
    I = fr.planes
    v = ((I[:, ymax, xmax] + I[:, ymin, xmin]) - I[:, ymax, xmin]) - I[:, ymin, xmax]
    n = np.zeros(m, np.int64); has = np.zeros(m, bool)
    nn = v[3].astype(np.int64)
    ok = (itv >= 0) & (nn >= conv["min_points"])
    n[pid] = np.where(ok, nn, 0); has[pid] = ok
    mean = np.zeros((m, 3), F32); cov = np.zeros((m, 3, 3), F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = np.where(v[3] != 0, F32(1.0) / v[3], F32(0)).astype(F32)
        mu = [(v[k] * d).astype(F32) for k in range(3)]
        ent = {(0, 0): v[4] * d - mu[0] * mu[0], (1, 0): v[5] * d - mu[1] * mu[0], (2, 0): v[6] * d - mu[2] * mu[0],
               (1, 1): v[7] * d - mu[1] * mu[1], (2, 1): v[8] * d - mu[2] * mu[1], (2, 2): v[9] * d - mu[2] * mu[2]}
    for k in range(3):
        mean[pid[ok], k] = mu[k][ok]
    for (i, j), e in ent.items():
        cov[pid[ok], i, j] = e[ok]; cov[pid[ok], j, i] = e[ok]
    return n, has, mean, cov


def eig_branches(O, cov):
    """which branches eig3_direct takes on these fp32 covariances: its first half restated in numpy fp32 (same operations, same order),
    the trig by the oracle's canonical evaluation"""
    with np.errstate(all="ignore"):
        a00, a10, a20, a11, a21, a22 = (cov[:, 0, 0], cov[:, 1, 0], cov[:, 2, 0], cov[:, 1, 1], cov[:, 2, 1], cov[:, 2, 2])
        shift = ((a00 + a11) + a22) / F32(3.0)
        S = [a00 - shift, a10, a20, a11 - shift, a21, a22 - shift]
        scale = np.max(np.abs(np.stack(S + [a10, a20, a21])), 0).astype(F32)
        sc = np.where(scale > 0, scale, F32(1))
        m00, m10, m20, m11, m21, m22 = [np.where(scale > 0, x / sc, x).astype(F32) for x in S[:1] + S[1:3] + S[3:4] + S[4:5] + S[5:6]]
        inv3 = F32(1.0) / F32(3.0)
        c0 = m00 * m11 * m22 + F32(2.0) * m10 * m20 * m21 - m00 * m21 * m21 - m11 * m20 * m20 - m22 * m10 * m10
        c1 = m00 * m11 - m10 * m10 + m00 * m22 - m20 * m20 + m11 * m22 - m21 * m21
        c2 = m00 + m11 + m22
        c2o3 = c2 * inv3
        a3 = (c2 * c2o3 - c1) * inv3
        half_b = F32(0.5) * (c0 + c2o3 * (F32(2.0) * c2o3 * c2o3 - c1))
        a3c = np.maximum(a3, F32(0))
        q = a3c * a3c * a3c - half_b * half_b
        qc = np.maximum(q, F32(0))
        rho = np.sqrt(a3c)
        th, ct, st = O.trig_eval(0, np.sqrt(qc), half_b)
        s3 = np.sqrt(F32(3.0))
        e0 = c2o3 - rho * (ct + s3 * st); e1 = c2o3 - rho * (ct - s3 * st); e2 = c2o3 + F32(2.0) * rho * ct
        eps = F32(np.finfo(np.float32).eps)
        iso = (e2 - e0) <= eps
        d0, d1 = e2 - e1, e1 - e0
        dmin = np.minimum(d0, d1); dmax = np.maximum(d0, d1)
        double = ~iso & (dmin <= F32(2) * eps * dmax)
        ev0 = (e0 * scale).astype(F32) + shift                          # e[0] * scale + shift, before the `ev[0] < 0` clamp
    return dict(scale_zero=scale == 0, a_over_3_clamped=a3 < 0, q_clamped=q < 0, half_b_zero=half_b == 0,
                half_b_neg_zero=(half_b == 0) & np.signbit(half_b), isotropic=iso, double_root=double, ev0_clamped=ev0 < 0,
                denormal_cov=((np.abs(cov) < np.finfo(np.float32).tiny) & (cov != 0)).reshape(len(cov), -1).any(1))


def bits_equal(a, b):
    """same bits, or both zero (+0 / -0: zero rows of the information matrices are built differently), or NaN in the same position"""
    a = np.asarray(a, F32); b = np.asarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))


def compare_to_oracle(o, g, sym6=False, skip=None):
    """every output field of a frame; returns {field: number of differing points}.  skip: points left out of every field but the points
    themselves (lean frames: the pixels of an undefined float-to-int conversion, whose window the two sides choose differently)"""
    bad = {}
    if skip is not None and skip.any():
        bad_pts = int((~bits_equal(o["points"], g["points"])).any(1).sum())
        keep = ~skip
        bad = compare_to_oracle({k: v[keep] for k, v in o.items()}, {k: v[keep] for k, v in g.items()}, sym6)
        bad["points"] = bad_pts
        return bad
    for k in ("points", "normals", "curvature", "omega_n", "eigenvalues"):
        bad[k] = int((~bits_equal(o[k].reshape(len(o[k]), -1), g[k].reshape(len(g[k]), -1))).any(1).sum())
    bad["npoints"] = int((o["npoints"] != g["npoints"]).sum())
    ok = o["npoints"] > 0
    st = ~bits_equal(o["stats"].reshape(-1, 16)[:, :15], g["stats"].reshape(-1, 16)[:, :15]).reshape(len(ok), -1).any(1)
    bad["stats (eigenvectors, mean)"] = int((st & ok).sum())
    op, gp = o["omega_p"].reshape(-1, 4, 4).transpose(0, 2, 1), g["omega_p"].reshape(-1, 4, 4).transpose(0, 2, 1)      # column-major -> [i, j]
    if sym6:
        up = np.triu_indices(3)
        bad["omega_p"] = int((~bits_equal(op[:, :3, :3][:, up[0], up[1]], gp[:, :3, :3][:, up[0], up[1]])).any(1).sum())
        lo = gp[:, :3, :3]
        bad["omega_p symmetric"] = int((~bits_equal(lo, lo.transpose(0, 2, 1))).reshape(len(lo), -1).any(1).sum())
        fin = np.isfinite(o["omega_p"]).all(1) & np.isfinite(g["omega_p"]).all(1)
        from test_omega_sym6 import compare_clouds_sym6          # the suite's sym6 comparison, on the points whose matrices are finite
        compare_clouds_sym6({k: o[k][fin] for k in ("points", "normals", "curvature", "omega_n", "omega_p")},
                            {k: g[k][fin] for k in ("points", "normals", "curvature", "omega_n", "omega_p")})
    else:
        bad["omega_p"] = int((~bits_equal(op, gp)).reshape(len(op), -1).any(1).sum())
    return bad


# ------------------------------------------------------------------------------------------------ against float64 (no oracle)
# Bars of the closed-form solver against float64 LAPACK on the same fp32 covariance, |d lambda| / lambda_max per family, measured on the
# CPU twin (test_stats_windows_cpu.py prints the worst values) and set with margin: the solver itself is that loose (the characteristic
# polynomial's roots in fp32), this is not a bug.  "dense": windows of an integral image of random points.
EIG_BARS = dict(distinct=3e-4, two_equal=3.5e-4, three_equal=1e-12, rank1=3.5e-4, rank2=1.5e-4, decades=3.5e-4, denormal=2.5e-4, zero=0.0,
                constant=0.0, far_off_centre=2.5e-4, curvature=1e-4, flip_zero=1e-4, n_edge=2.5e-4, combine=2.5e-4, itv_neg=2.5e-4, dense=2e-4,
                dense_raw=5e-5)
NORMAL_K = 1.5e-3     # normal angle <= NORMAL_K * lambda_max / eigen-gap (+ NORMAL_ABS): the solver's bound over the gap
NORMAL_ABS = 1e-5
DENORM_ABS = 8 * 2.0 ** -149


def check_against_float64(frames, outs, conv, offset=False, pflat=(1000.0, 1.0, 1.0), nflat=100.0, nnonflat=1.0):
    """the three steps of test_gpu_stats_against_numpy_fp32_sums_and_lapack on adversarial windows; `outs` are the implementation's arrays
    (GPU or oracle).  Returns the report; raises AssertionError on a failure."""
    rep = dict(windows={}, worst_eig={}, worst_normal=0.0, near_threshold=0)
    f32 = F32
    for fr, a in zip(frames, outs):
        n, has, mean, cov = window_cov(fr, conv)
        # 1. count and mean bit for bit
        assert np.array_equal(a["npoints"], n), "window counts differ from numpy"
        gmean = a["stats"].reshape(-1, 16)[:, 12:15]
        if not offset:
            assert np.array_equal(gmean[has].view(np.uint32), mean[has].view(np.uint32)), "window means differ from numpy fp32"
        sel = np.nonzero(has & np.isfinite(cov).reshape(len(cov), -1).all(1))[0]
        w, V = np.linalg.eigh(cov[sel].astype(np.float64))
        ev = a["eigenvalues"][sel].astype(np.float64)
        lam = np.abs(w).max(1)
        err = np.maximum(np.abs(np.maximum(w[:, 0], 0) - ev[:, 0]), np.abs(w[:, 1:] - ev[:, 1:]).max(1))
        err = np.maximum(err - DENORM_ABS, 0)                  # fp32 results below FLT_MIN sit on a grid of 2^-149
        rel = np.where(lam > 0, err / np.where(lam > 0, lam, 1), err)
        fam = fr.family[sel]
        for name in np.unique(fam):
            k = fam == name
            rep["windows"][name] = rep["windows"].get(name, 0) + int(k.sum())
            worst = float(rel[k].max())
            rep["worst_eig"][name] = max(rep["worst_eig"].get(name, 0.0), worst)
            assert worst <= EIG_BARS[name], f"{name}: |d lambda| / lambda_max {worst:.2e} above the bar {EIG_BARS[name]:.1e}"
        # 2. normals against LAPACK's, where the eigen-gap separates them
        U = a["stats"].reshape(-1, 4, 4)[sel].transpose(0, 2, 1)[:, :3, :3].astype(np.float64)
        gap = w[:, 1] - w[:, 0]
        good = (gap > 1e-2 * lam) & (lam > 0) & np.isfinite(U).all((1, 2))
        if not offset and good.any():
            cosang = np.abs((U[good, :, 0] * V[good, :, 0]).sum(1))
            ang = np.arccos(np.clip(cosang, 0, 1))
            tol = NORMAL_K * lam[good] / gap[good] + NORMAL_ABS
            assert (ang <= tol).all(), f"normal angle {float(ang.max()):.2e}, worst angle / bar {float((ang / tol).max()):.2f}"
            rep["worst_normal"] = max(rep["worst_normal"], float((ang / tol).max()))
        if offset:
            continue
        # 3. what follows the eigen-solve, from the implementation's own eigenvalues / eigenvectors, bit for bit
        evf = a["eigenvalues"][sel]
        Uf = a["stats"].reshape(-1, 4, 4)[sel].transpose(0, 2, 1)[:, :3, :3]
        with np.errstate(all="ignore"):
            curv = (evf[:, 0].astype(np.float64) / ((evf[:, 0] + evf[:, 1] + evf[:, 2]).astype(f32).astype(np.float64) + 1e-9)).astype(f32)
        assert np.array_equal(a["curvature"][sel].view(np.uint32), curv.view(np.uint32)), "curvature differs from numpy on the same eigenvalues"
        keep = curv < f32(conv["stats_curvature_threshold"])
        nrm = a["normals"][sel, :3]
        assert np.array_equal(np.abs(nrm).sum(1) > 0, keep & (np.abs(Uf[:, :, 0]).sum(1) > 0)), "normal survival"
        P = fr.points[sel, :3]
        u0 = Uf[:, :, 0]
        dp = ((u0[:, 0] * P[:, 0] + u0[:, 1] * P[:, 1]) + u0[:, 2] * P[:, 2]) + f32(0.0) * f32(1.0)
        want = np.where((dp > 0)[:, None], -u0, u0)
        assert bits_equal(nrm[keep], want[keep]).all(), "normal flip"
        flat = curv < f32(conv["point_info_curvature_threshold"])
        with np.errstate(all="ignore"):
            dg = np.where(flat[:, None], np.array(pflat, f32)[None, :], f32(1.0) / evf).astype(f32)
            om = np.zeros((len(sel), 3, 3), f32)
            for i in range(3):
                for j in range(3):
                    om[:, i, j] = ((Uf[:, i, 0] * dg[:, 0]) * Uf[:, j, 0] + (Uf[:, i, 1] * dg[:, 1]) * Uf[:, j, 1]) + (Uf[:, i, 2] * dg[:, 2]) * Uf[:, j, 2]
        gom = a["omega_p"][sel].reshape(-1, 4, 4).transpose(0, 2, 1)[:, :3, :3]
        up = np.triu_indices(3)
        live = keep & (np.abs(nrm).sum(1) > 0)
        assert bits_equal(gom[live][:, up[0], up[1]], om[live][:, up[0], up[1]]).all(), "omega_p"
        assert not gom[~live].any(), "omega_p of a dropped normal"
        gon = a["omega_n"][sel].reshape(-1, 4, 4).transpose(0, 2, 1)[:, :3, :3]
        cls = curv < f32(conv["normal_info_curvature_threshold"])
        want_n = np.where(cls[:, None, None], np.eye(3, dtype=f32) * f32(nflat), np.eye(3, dtype=f32) * f32(nnonflat))
        assert np.array_equal(gon[live], want_n[live]) and not gon[~live].any(), "omega_n class"
        # decisions against float64's: equal except within the eigenvalue bar of a threshold
        w0 = np.maximum(w[:, 0], 0); tot = w.sum(1)
        c64 = w0 / (tot + 1e-9)                                 # Stats::curvature's + 1e-9 (stats.h:98-103)
        bar = (np.array([EIG_BARS[f] for f in fam]) * lam + DENORM_ABS) * 3 / (tot + 1e-9)
        for key in THRESHOLDS:
            t = float(f32(conv[key]))
            near = np.abs(c64 - t) <= bar
            mism = ((curv < f32(t)) != (c64 < t)) & (tot > 0)
            assert not (mism & ~near).any(), f"{key}: {int((mism & ~near).sum())} decisions differ from float64 away from the threshold"
            rep["near_threshold"] += int((mism & near).sum())
    return rep
