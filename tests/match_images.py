"""Injected depth pairs for the matchClouds score (k_match_score; pwn_tracker/pwn_matcher_base.cpp:153-182) and an integer model of it.

The model is written from the reference's lines, not from the kernel:

    c, r    = uint16(float32(1000) * depth), FLT_MAX -> 0                      (:157,160  DepthImage_convert_32FC1_to_16UC1)
    mask    = c > 0 and r > 0                                                  (:163)
    d       = float32(|c - r|) with its WORD and-ed with bits(255.0f) = 0x437F0000   (:164-167: cv::Mat `abs(a - b) & mask` on CV_32F data)
    counts  = nonZeros = #mask, inliers = #(mask and d < threshold), outliers = nonZeros - inliers                          (:168,174-175,180-182)
    sum     = the sum of d over the image, kept as an exact Python integer in units of 2^-121                               (:176)
    distance = float32(sum) / float32(nonZeros)                                                                             (:179)

The and keeps the exponent bits 10000110b (134) and the upper seven mantissa bits, so a difference falls into one of these classes
(`classes`, counted on the uint16 values, not on the millimetres a builder intended):

    0           d = 0
    1           exponent 127 & 134 = 6: d = 2^-121 -- not zero, and below every inlier threshold > 0
    2-3         exponent 128 stays: d = the difference
    4-7         exponent 129 -> 128: halved (shift class 128)
    8-31        -> exponent 130: 8-15 kept, 16-31 halved (shift class 130)
    32-127      -> exponent 132 (shift class 132)
    128-511     -> exponent 134; 256-511 lose their last mantissa bit as well (shift class 134)
    512-1023    exponent 136 -> 128: folded back into [2, 4) in steps of 1/64
    >= 1024     exponent 137.. -> 128, 130, ..: folded back

Every d is 0, 2^-121 or a multiple of 1/64, hence the unit.  The reference adds the image up sequentially in float: below 2^18 mm such a sum of
multiples of 1/64 is exact (2^18 * 64 = 2^24) and the 2^-121 terms vanish next to anything else, so `float32(sum)` of the exact integer IS the
reference's sum (BITWISE pairs).  Above that its partial sums round: n - 1 additions of non-negative terms, each off by at most 2^-24 of the
partial sum, itself at most the total -- (n - 1) * 2^-24 relative (`long_sum_bar`).

The builder: hand-made frames whose per-pixel difference is under control.  Depths are float32((raw + 0.5) / 1000): 1000 * that is raw + 0.5
up to a few 1e-4, so the uint16 cast gives raw (0.001f * raw does not: 1000 * it truncates to raw - 1 for some raw).  The camera maps the
unprojected point of a pixel back onto that pixel with its depth unchanged (asserted in tests/test_match_images_cpu.py), so under an
identity guess the finder's images are the frames."""
from collections import Counter, namedtuple
from fractions import Fraction

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
MIN_DISTANCE, MAX_DISTANCE = 0.5, 6.0                  # max_distance <= 60 m: the uint16 cast of larger depths is undefined in the reference
WG = 256                                               # work-items of a k_match_score workgroup (what the shapes are chosen against)
BATCH_SHAPE = (132, 160)                               # 21 120 pixels = 82.5 workgroups: a 64-workgroup launch takes a second, partial turn
SINGLE_SHAPE = (264, 256)                              # 67 584 pixels = 264 workgroups: the single-pair entry's 256-workgroup cap takes a second turn
TABLE_SHAPE = (24, 32)
TINY_EXP = 121                                         # bits(1.0f) & bits(255.0f) = 0x03000000 = 2^-121
UNIT = Fraction(1, 2 ** TINY_EXP)
BITWISE_SUM_MM = 2 ** 18
CLASSES = ("0", "1", "2-3", "4-7", "8-31", "32-127", "128-511", "512-1023", ">=1024")
# one value or more from every class; 516 -> 2 + 1/64 (an odd number of 1/64), 257 loses its last bit, 2048.. lands in shift class 130
DELTAS = (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 49, 50, 51, 63, 64, 65, 100, 127, 128, 200, 255, 256, 257, 300, 511, 512, 516, 600, 1023, 1024, 2000,
          2048, 3000)
SMALL = (0, 1, 2, 3, 0, 1, 0, 2)

Pair = namedtuple("Pair", "name kind ref cur")         # frames: float32 [rows, cols] metres, 0 = no measurement


def camera(rows, cols):
    """(fx, fy, cx, cy) of a camera that sees the whole image"""
    return (float(cols) * 0.75, float(cols) * 0.75, (cols - 1) / 2.0, (rows - 1) / 2.0)


def converter_conf():
    """converter parameters for the frames (the reference's imageScale-4 radii: small images)"""
    return dict(min_distance=MIN_DISTANCE, max_distance=MAX_DISTANCE, world_radius=0.1, min_image_radius=3, max_image_radius=6, min_points=10,
                stats_curvature_threshold=0.2, point_info_curvature_threshold=0.02, normal_info_curvature_threshold=0.02)


def aligner_conf(outer_iterations=1):
    return dict(min_distance=MIN_DISTANCE, max_distance=MAX_DISTANCE, inlier_distance_threshold=0.5, inlier_normal_angular_threshold=0.95,
                flat_curvature_threshold=0.02, inlier_curvature_ratio_threshold=1.3, inlier_max_chi2=9000.0, robust_kernel=1,
                outer_iterations=outer_iterations, inner_iterations=1)


# ---------------------------------------------------------------------------------------------------- the model
def to_u16(depth):
    """DepthImage_convert_32FC1_to_16UC1 with scale 1000: FLT_MAX -> 0, else the truncating cast of float32(1000) * d (d <= 60 m)"""
    d = np.asarray(depth, F)
    v = F(1000.0) * np.where(d < FLT_MAX, d, F(0))
    assert float(v.max(initial=0.0)) < 65536.0 and float(v.min(initial=0.0)) >= 0.0
    return v.astype(np.int64).astype(np.uint16)


def masked_words(ref_depth, cur_depth):
    """(mask, words of d, |c - r| in uint16 millimetres) per pixel"""
    c, r = to_u16(cur_depth).reshape(-1), to_u16(ref_depth).reshape(-1)
    mask = (c > 0) & (r > 0)
    diff = np.abs(c.astype(np.int64) - r.astype(np.int64))
    words = diff.astype(F).view(np.uint32) & np.uint32(0x437F0000)
    return mask, np.where(mask, words, np.uint32(0)).astype(np.uint32), np.where(mask, diff, 0)


def units_of(words):
    """the value of every masked word as an exact integer number of 2^-121 (Python ints in an object array)"""
    out = []
    for w in np.unique(words):
        e, m = int(w) >> 23, int(w) & 0x7FFFFF
        v = Fraction(0) if w == 0 else Fraction((1 << 23) + m, 1 << 23) * (Fraction(2) ** (e - 127))
        q = v / UNIT
        assert q.denominator == 1
        out.append((int(w), q.numerator))
    return dict(out)


def f32_of(frac):
    """round-to-nearest-even float32 of an exact non-negative Fraction"""
    if frac == 0:
        return F(0.0)
    n, d = frac.numerator, frac.denominator
    e = n.bit_length() - d.bit_length()
    if Fraction(2) ** e > frac:
        e -= 1
    assert -126 <= e <= 127                                            # normal range
    q = frac / (Fraction(2) ** (e - 23))                               # in [2^23, 2^24)
    k, rem = divmod(q.numerator, q.denominator)
    twice = 2 * rem
    if twice > q.denominator or (twice == q.denominator and (k & 1)):
        k += 1
    return F(np.ldexp(float(k), e - 23))


def score(ref_depth, cur_depth, threshold):
    """dict(nonZeros, inliers, outliers, sum_units (exact, units of 2^-121), sum_mm (float64, for the bounds), distance (float32; NaN for 0/0))"""
    mask, words, _ = masked_words(ref_depth, cur_depth)
    d = words.view(F)
    nz = int(mask.sum())
    inl = int((mask & (d < F(threshold))).sum())
    val = units_of(words)
    cnt = Counter(words.tolist())
    total = sum(val[w] * k for w, k in cnt.items())
    s = f32_of(total * UNIT)
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = F(s) / F(nz)
    return dict(nonZeros=nz, inliers=inl, outliers=nz - inl, sum_units=total, sum_mm=float(total * UNIT), distance=F(dist))


def classes(ref_depth, cur_depth):
    """Counter of the classes of the module text over the common valid pixels"""
    mask, _, diff = masked_words(ref_depth, cur_depth)
    d = diff[mask]
    edges = [(0, 0), (1, 1), (2, 3), (4, 7), (8, 31), (32, 127), (128, 511), (512, 1023), (1024, 1 << 20)]
    return Counter({name: int(((d >= lo) & (d <= hi)).sum()) for name, (lo, hi) in zip(CLASSES, edges)})


def long_sum_bar(n_common):
    """relative bound of the reference's sequential float sum of n non-negative terms against the exact sum"""
    return max(0, n_common - 1) * 2.0 ** -24


def bits(x):
    return int(np.asarray(x, F).reshape(1).view(np.uint32)[0])


def same_distance(a, b):
    """bit for bit, any NaN equal to any NaN (the sign of 0/0 differs between hosts)"""
    a, b = F(a), F(b)
    return bool(np.isnan(a) and np.isnan(b)) or bits(a) == bits(b)


# ---------------------------------------------------------------------------------------------------- the builder
def _depth(raw):
    return ((np.asarray(raw, np.float64) + 0.5) / 1000.0).astype(F)


def _base(rows, cols, seed):
    """reference raw millimetres: a tilted plane with a seed-dependent offset, 1.2 .. 2.6 m"""
    r, c = np.mgrid[0:rows, 0:cols]
    return (1200 + 53 * (seed % 11) + (3 * r + 2 * c) % 700).astype(np.int64)


def _deltas(rows, cols, seed, rare):
    """per-pixel signed difference: SMALL everywhere, a DELTAS entry at every `rare`-th pixel; the sign alternates below 512 mm"""
    i = np.arange(rows * cols, dtype=np.int64)
    small = np.asarray(SMALL, np.int64)[(i * 5 + seed) % len(SMALL)]
    full = np.asarray(DELTAS, np.int64)[((i // max(rare, 1)) * 7 + seed) % len(DELTAS)]
    d = np.where((i + seed) % max(rare, 1) == 0, full, small)
    sign = np.where((d < 512) & ((i // 3) % 2 == 1), -1, 1)
    return (d * sign).reshape(rows, cols)


def _holes(ref, cur, seed, tail_rows):
    rows, cols = ref.shape
    r0, c0 = 5 + (seed * 7) % (rows - 20), 3 + (seed * 11) % (cols - 30)
    ref[r0:r0 + 4, c0:c0 + 10 + seed % 13] = 0                         # reference side only ...
    cur[r0 + 2:r0 + 9, c0 + 5:c0 + 12 + (seed * 5) % 17] = 0           # ... both sides where they overlap, current side only
    cur[(r0 + 11) % rows, :] = 0
    if tail_rows:                                                      # the last rows: the tail workgroups contribute nothing
        ref[rows - tail_rows:, :] = 0
        cur[rows - 1:, : cols // 2] = 0


def sum64(ref_depth, cur_depth):
    """(the sum of the differences that survive as multiples of 1/64, in 1/64; the number of 1 mm pixels)"""
    mask, words, diff = masked_words(ref_depth, cur_depth)
    val = units_of(words)
    ones = int((mask & (diff == 1)).sum())
    total = sum(val[w] * k for w, k in Counter(words.tolist()).items()) - ones
    assert total % (1 << (TINY_EXP - 6)) == 0
    return total >> (TINY_EXP - 6), ones


def is_tie(s64, down=False):
    """the sum lies exactly half-way between two neighbouring floats (down: and the even one of them is the lower)"""
    sh = s64.bit_length() - 24
    return sh >= 1 and (s64 & ((1 << sh) - 1)) == (1 << (sh - 1)) and not (down and (s64 >> sh) & 1)


def _tip_to_tie(ref, cur):
    """the long sum: a few 0 mm pixels become 516 mm (129/64 each, an odd number) until the 1/64 part of the sum is a tie -- its float
    rounds to even (downwards) on its own and upwards with the 1 mm pixels of the pair added, so the exact sum and the 1/64 part differ in the last bit"""
    mask, _, diff = masked_words(ref, cur)
    zeros = np.flatnonzero(mask & (diff == 0))
    raw = to_u16(ref).reshape(-1).astype(np.int64)
    for i in zeros[:64]:
        if is_tie(sum64(ref, cur)[0], down=True):
            return
        cur.reshape(-1)[i] = _depth(raw[i] + 516)
    assert is_tie(sum64(ref, cur)[0], down=True)


def class_pair(rows, cols, seed, rare=37, tail_rows=0, name=None):
    """every class, holes on either and on both sides; rare: every how many pixels a large difference stands (1: all of them -- the long sum)"""
    raw = _base(rows, cols, seed)
    ref, cur = _depth(raw), _depth(raw + _deltas(rows, cols, seed, rare))
    _holes(ref, cur, seed, tail_rows)
    kind = "long" if rare == 1 else "bitwise"
    if kind == "long":
        _tip_to_tie(ref, cur)
    return Pair(name or f"{kind}/{rows}x{cols}/s{seed}" + (f"/tail{tail_rows}" if tail_rows else ""), kind, ref, cur)


def one_mm_pair(rows, cols, seed=0):
    """all common pixels differ by exactly 0 or 1 mm"""
    raw = _base(rows, cols, seed)
    i = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    ref, cur = _depth(raw), _depth(raw + np.where((i + seed) % 3 == 0, 1, 0) * np.where(i % 2 == 0, 1, -1))
    _holes(ref, cur, seed + 2, 0)
    return Pair(f"one_mm/{rows}x{cols}/s{seed}", "one_mm", ref, cur)


def tail_pair(rows, cols, seed=0):
    """the current frame holds two pixels only: the very last one and one more in the partial tail workgroup"""
    n = rows * cols
    assert n % WG != 0
    raw = _base(rows, cols, seed)
    ref = _depth(raw)
    cur = np.zeros((rows, cols), F)
    first_tail = (n // WG) * WG
    for i, delta in ((n - 1, 5), (first_tail + (n - first_tail) // 3, 1)):
        cur.reshape(-1)[i] = _depth(raw.reshape(-1)[i] + delta)
    return Pair(f"tail/{rows}x{cols}/s{seed}", "tail", ref, cur)


def empty_pair(rows, cols, seed=0):
    """no common valid pixel: the reference frame holds the left half, the current frame the right"""
    raw = _base(rows, cols, seed)
    ref, cur = _depth(raw), _depth(raw + 2)
    ref[:, cols // 2:] = 0
    cur[:, : cols // 2] = 0
    return Pair(f"empty/{rows}x{cols}/s{seed}", "empty", ref, cur)


def table_pair():
    """the hand-readable class table: column k of a 24 x 32 image differs by the k-th of 32 DELTAS entries"""
    rows, cols = TABLE_SHAPE
    raw = np.full((rows, cols), 1500, np.int64)
    d = np.array([x for x in DELTAS if x not in (49, 51, 65, 200)], np.int64)
    assert len(d) == cols
    ref, cur = _depth(raw), _depth(raw + d[None, :])
    ref[3, :] = 0; cur[5, 4:9] = 0; ref[5, 7:12] = 0
    return Pair("table/24x32", "bitwise", ref, cur)


_cache = {}


def batch_pairs(n):
    """n pairs of BATCH_SHAPE with n distinct scores: the tail pair, the empty pair, the 1 mm pair and the long sum among class pairs"""
    if n not in _cache:
        rows, cols = BATCH_SHAPE
        special = [tail_pair(rows, cols, 1), empty_pair(rows, cols, 2), class_pair(rows, cols, 3, tail_rows=3)]
        if n > 3:
            special += [one_mm_pair(rows, cols, 4), class_pair(rows, cols, 5, rare=1), class_pair(rows, cols, 6)]
        out = list(special)
        seed = 7
        while len(out) < n:
            out.append(class_pair(rows, cols, seed, rare=29 + 2 * (seed % 5), tail_rows=3 * (seed % 2)))
            seed += 1
        _cache[n] = out[:n]
    return _cache[n]


def single_pair():
    if "single" not in _cache:
        _cache["single"] = class_pair(*SINGLE_SHAPE, seed=9, rare=41)
    return _cache["single"]


def guess(kind):
    """identity, or a small rotation and translation (z translation 0, as matchClouds conditions its guess, pwn_matcher_base.cpp:114)"""
    T = np.eye(4, dtype=F)
    if kind == "identity":
        return T
    assert kind == "moved"
    a, b = 0.011, -0.007
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    T[:3, :3] = (Rz @ Ry).astype(F)
    T[:3, 3] = (0.013, -0.008, 0.0)
    return T
