"""Injected points for PinholePointProjector::project in every launch form of the library: the stand-alone projection (k_project_single +
k_zbuf_resolve), the aligner's latency and throughput launches (k_project<1>, k_project<4> with z32_settle), its two-pass form
(k_project_robust), the depth-only batch (k_project_depth_batch) and the host's single-point form (pwn_hip_project_point).  A helper module of
the tests, imported by test_project_points_cpu.py and test_gpu_project_points.py.

Usage of this tree: the MODEL is numpy_reference_model.project with oracle.projector_matrices, fp32 in the reference's operation order; the
ORACLE is oracle.project.  A float64 evaluation of the same expression only LABELS points: a decision is "made by rounding" where the fp32
pixel or acceptance differs from the float64 one.  summary() prints those counts.

A case holds points, a family / sub label per point, an image size, K, the range and a projector transform T.  Under the identity the
generators evaluate the tested quantity in fp32 in the reference's order and keep what hits an edge exactly (and its nearest attainable
neighbours); under the transforms `small` and `moderate` of align_clouds.GUESSES the camera-frame point is carried through T in float64,
rounded, and edges are met by log-spaced ladders (1e-7.5 .. 1e-3 either side).  Points are stored in a seeded permutation except where a
label fixes the index.  Per point `expect` says what the images must show: PRESENT (the point's index at `pixel`), ABSENT (its index
nowhere) or OPEN (a ladder step too close to an edge to be called without the fp32 expression itself: only model == oracle == GPU is asked).

Families and their sub labels (REPEAT = 8 points per sub label unless stated):
  round_tie   col<t>/tie, col<t>/below(<u>ulp), col<t>/above(<u>ulp), row<t>/...: t = k + 0.5, k in {-1, 0, 1, 7, middle, size - 2, size - 1};
              u = distance of the nearest attainable value from t in float32 steps.  The (x, z) pairs that reach a value are few: the REPEAT
              points of a label reuse them on REPEAT different lines of the other axis.  Ladder cases: col<t>/-1e-05 ... (one point per step).
  depth_edge  min<k>ulp / max<k>ulp, k = -2 .. 2, for the ranges (0.5, 5.0) and (0, 6.0); ladder cases min-1e-05 ...
  behind      negative, plus_zero, minus_zero, denormal (min_distance = 0): nothing lands.
  collide     equal<m>, near_high<m>, near_low<m> for m in 2, 3, 4, 64, 65, 300 (one group each, m points); own_thread/near_last,
              own_thread/equal (indices i, i + 256, i + 512, i + 768); one_wave/equal, one_wave/near_high (64 consecutive indices);
              cross_wg/near_high, cross_wg/equal (indices 1030 apart); under `moderate`: recomputed/equal (8 times the same world point),
              recomputed/ladder.
  sizes       clouds of 0 .. 2049 points, one per pixel while the pixels last, then again at other depths; each under its own small transform.
  far         finite points whose pixel lies beyond +-2^31, inf and NaN coordinates: model only (the reference's int conversion is undefined).
  fill        points behind the camera that pad a cloud up to an index a label needs.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_clouds as A      # noqa: E402
import numpy_reference_model as M      # noqa: E402

F32 = np.float32
F64 = np.float64
REPEAT = 8
OPEN, PRESENT, ABSENT = 0, 1, 2
FLT_MAX = np.finfo(F32).max
CAMERAS = {"wide": (24, 32, (30.0, 30.0, 15.5, 11.5)), "tele": (23, 41, (525.0, 525.0, 20.0, 11.0))}
RANGES = ((0.5, 5.0), (0.0, 6.0))
SIZES = (0, 1, 255, 256, 257, 1023, 1024, 1025, 2049)
SIZES_CAPACITY = 3072              # the roomy clouds of the sizes: whole workgroups of 4 x 256 points, so every index the grid can form lies inside the arrays
COLLIDE_POINTS = 2304
GROUPS = (2, 3, 4, 64, 65, 300)
VARIANTS = ("div", "rint", "trunc", "fma", "min_le", "max_ge", "edge_le", "neg_zero", "tie_high", "first_wins")
ULPS = 24                         # candidates either side of the float64 solution of a tie
SEARCH_DEPTHS = 256               # ten round depths and random ones: an exact tie needs the right (x, z) pair, see the module text
LADDER = 10.0 ** np.linspace(-7.5, -3.0, 10)
# A float64 decision further than this from its edge is the fp32 one too.  The terms of an image row stay below 150 here (the tele camera's
# K t under `moderate` is the largest), so its four roundings and the two of the quotient move the fp32 pixel value by less than 6 * 150 * 2^-24
# = 5.4e-5 at the ladders' depths (>= 1); the depth row's terms stay below 3 d: less than 1e-6 relative.  Pixels off a ladder sit on centres.
MARGIN_PIXEL, MARGIN_DEPTH = 1e-4, 1e-5
SATURATED = 2147483520            # what pwn_hip_project_point returns for a rounded coordinate an int cannot hold (include/pwn_hip.h)
INT_MIN = -2 ** 31                # ... and for a NaN


class Case:
    def __init__(self, **kw):
        self.ask_oracle = True
        self.__dict__.update(kw)
        self._krt = None

    @property
    def n(self):
        return len(self.P)

    @property
    def key(self):
        """cases of one key can share a launch of the batch forms"""
        return (self.rows, self.cols, self.K, self.min_d, self.max_d, self.name.startswith("sizes"))

    def points4(self):
        return np.concatenate([self.P, np.ones((self.n, 1), F32)], 1)

    def label(self, i):
        return f"{self.family[i]}/{self.sub[i]}"


def krt(case):
    if case._krt is None:
        from oracle import oracle as O
        case._krt = O.projector_matrices(case.K, case.T)[0]
    return case._krt


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def ordered(a):
    """float32 -> integers that order like the values (-0 and +0 both 0)"""
    b = np.asarray(a, F32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def ulp_step(x, k):
    """x moved by k float32 steps towards +inf (k < 0: towards -inf); no step crosses zero"""
    o = ordered(x) + np.asarray(k, np.int64)
    assert np.all((o > 0) == (np.asarray(x) > 0)) or np.all(np.asarray(x) == 0)
    b = np.where(o < 0, (-o) | 0x80000000, o)
    return b.astype(np.uint32).view(F32)


def ulp_step0(edge, k):
    """the same from an edge that may be zero"""
    v = F32(edge)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf), dtype=F32)
    return v


# ------------------------------------------------------------------------------------------------------------------------ the model
def plane(P, KRt, variant=None):
    """ip = KRt * (x, y, z, 1), each row (((a0 x + a1 y) + a2 z) + a3 1) in fp32; variant "fma": every sum contracted with its product"""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    one = np.ones(len(P), F32)

    def row(r):
        if variant != "fma":
            return ((KRt[r, 0] * x + KRt[r, 1] * y) + KRt[r, 2] * z) + KRt[r, 3] * F32(1.0)
        s = KRt[r, 0] * x
        for a, b in ((KRt[r, 1], y), (KRt[r, 2], z), (KRt[r, 3], one)):
            s = (s.astype(F64) + F64(a) * b.astype(F64)).astype(F32)
        return s
    return row(0), row(1), row(2)


def project(P, KRt, min_d, max_d, rows, cols, variant=None):
    """numpy_reference_model.project, or one of the wrong projections of VARIANTS -> (index image, depth image)"""
    P = np.ascontiguousarray(P, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        if variant is None:
            return M.project(P, KRt, min_d, max_d, rows, cols)
        ix, iy, d = plane(P, KRt, variant)
        lo = d <= F32(min_d) if variant == "min_le" else d < F32(min_d)
        hi = d >= F32(max_d) if variant == "max_ge" else d > F32(max_d)
        ok = ~(lo | hi)
        if variant == "div":
            vx, vy = ix / d, iy / d
        else:
            inv = F32(1.0) / d
            vx, vy = ix * inv, iy * inv
        rnd = {"rint": np.rint, "trunc": lambda v: np.trunc(v + F32(0.5))}.get(variant, M.roundf)
        rx, ry = rnd(vx).astype(F32), rnd(vy).astype(F32)
        if variant == "edge_le":
            ok &= (rx >= 0) & (rx <= cols) & (ry >= 0) & (ry <= rows)
        else:
            ok &= (rx >= 0) & (rx < cols) & (ry >= 0) & (ry < rows)
        if variant == "neg_zero":
            ok &= ~(((rx == 0) & np.signbit(rx)) | ((ry == 0) & np.signbit(ry)))
    idx = np.nonzero(ok)[0]
    pix = ry[idx].astype(np.int64) * cols + rx[idx].astype(np.int64)
    keep = pix < rows * cols                  # edge_le: a word behind the image belongs to nobody
    idx, pix = idx[keep], pix[keep]
    if variant == "first_wins":
        order = np.lexsort((idx, pix))
    elif variant == "tie_high":
        order = np.lexsort((-idx, d[idx], pix))
    else:
        order = np.lexsort((idx, d[idx], pix))
    pix_s, idx_s = pix[order], idx[order]
    first = np.ones(len(pix_s), bool); first[1:] = pix_s[1:] != pix_s[:-1]
    wi = np.full(rows * cols, -1, np.int32); wd = np.full(rows * cols, FLT_MAX, F32)
    wi[pix_s[first]] = idx_s[first]; wd[pix_s[first]] = d[idx_s[first]]
    return wi.reshape(rows, cols), wd.reshape(rows, cols)


def model_images(case, variant=None):
    return project(case.P, krt(case), case.min_d, case.max_d, case.rows, case.cols, variant)


def empty_images(case):
    return np.full((case.rows, case.cols), -1, np.int32), np.full((case.rows, case.cols), FLT_MAX, F32)


def changed_pixels(case, variant, family=None):
    """pixels whose index or depth word differs between the model and its variant; family: only pixels one of whose two winners belongs to it"""
    mi, md = model_images(case)
    vi, vd = model_images(case, variant)
    diff = (mi != vi) | (bits(md) != bits(vd))
    if family is not None:
        fam = np.concatenate([case.family == family, [False]])       # index -1 -> False
        diff &= fam[mi] | fam[vi]
    return int(diff.sum())


def single_points(case):
    """per point what the single-point form returns before the image-bounds test: (accepted by the range, d, rounded x, rounded y as floats)"""
    with np.errstate(all="ignore"):
        ix, iy, d = plane(case.P, krt(case))
        ok = ~((d < F32(case.min_d)) | (d > F32(case.max_d)))
        inv = F32(1.0) / d
        return ok, d, M.roundf(ix * inv), M.roundf(iy * inv)


def float64_decisions(case):
    """the same expression in float64 on the fp32 matrix and points -> (accepted, row, col, clear): clear = further than the margins from every edge"""
    K4 = krt(case).astype(F64); P = case.P.astype(F64)
    with np.errstate(all="ignore"):
        ip = P @ K4[:3, :3].T + K4[:3, 3]
        d = ip[:, 2]
        vx, vy = ip[:, 0] / d, ip[:, 1] / d
        rx, ry = np.floor(np.abs(vx) + 0.5) * np.sign(vx), np.floor(np.abs(vy) + 0.5) * np.sign(vy)
        in_range = ~((d < case.min_d) | (d > case.max_d))
        ok = in_range & (rx >= 0) & (rx < case.cols) & (ry >= 0) & (ry < case.rows)
        fr = lambda v: np.abs(np.abs(v - np.floor(v)) - 0.5)      # noqa: E731  distance from a rounding tie
        clear = np.isfinite(vx) & np.isfinite(vy) & (fr(vx) > MARGIN_PIXEL) & (fr(vy) > MARGIN_PIXEL)
        for e in (case.min_d, case.max_d):
            clear &= np.abs(d - e) > MARGIN_DEPTH * max(e, 1.0)
        clear &= np.abs(d) > 1e-3
        clear |= (d < -1e-3)                                        # well behind the camera: rejected whatever the pixel
    row = np.where(ok, ry, -1).astype(np.int64); col = np.where(ok, rx, -1).astype(np.int64)
    return ok, row, col, clear


def rounding_decisions(case):
    """points whose fp32 acceptance or pixel differs from the float64 one"""
    ok64, r64, c64, _ = float64_decisions(case)
    ok, d, fx, fy = single_points(case)
    with np.errstate(all="ignore"):
        ok32 = ok & (fx >= 0) & (fx < case.cols) & (fy >= 0) & (fy < case.rows)
        r32 = np.where(ok32, fy, -1).astype(np.int64); c32 = np.where(ok32, fx, -1).astype(np.int64)
    return int(((ok32 != ok64) | (r32 != r64) | (c32 != c64)).sum())


# ------------------------------------------------------------------------------------------------------------------------ building
class _Builder:
    def __init__(self, name, camera, rng_range, guess, seed):
        self.name, self.camera, self.guess = name, camera, guess
        self.rows, self.cols, self.K = CAMERAS[camera]
        self.min_d, self.max_d = rng_range
        self.T64 = np.asarray(A.GUESSES[guess] if isinstance(guess, str) else guess, F64)
        self.exact = isinstance(guess, str) and guess == "identity"
        self.rng = np.random.default_rng(seed)
        self.recs = []                   # (camera-frame point float64[3] or world float32[3], family, sub, expect, row, col, fixed index or -1, group id)
        self.used = {}                   # line of the other axis last handed out per (axis, line)
        self.free = [(r, c) for r in range(self.rows) for c in range(self.cols)]
        self.rng.shuffle(self.free)
        self.groups = 0

    def ray(self, r, c, z):
        """camera-frame point of depth z on the ray through the centre of pixel (r, c) (float64)"""
        fx, fy, cx, cy = self.K
        return np.array([(c - cx) * z / fx, (r - cy) * z / fy, z], F64)

    def add(self, cam, family, sub, expect=OPEN, pixel=(-1, -1), index=-1, group=-1, world=None):
        self.recs.append((cam, family, sub, expect, pixel[0], pixel[1], index, group, world))

    def pixel(self):
        return self.free.pop()

    def finish(self, n=None, shuffle=True):
        m = len(self.recs)
        n = m if n is None else n
        assert n >= m, (self.name, n, m)
        slots = np.full(n, -1, np.int64)
        fixed = [(k, r[6]) for k, r in enumerate(self.recs) if r[6] >= 0]
        for k, i in fixed:
            assert slots[i] < 0
            slots[i] = k
        rest = [k for k, r in enumerate(self.recs) if r[6] < 0]
        holes = np.nonzero(slots < 0)[0]
        if shuffle:
            self.rng.shuffle(holes)
        slots[holes[:len(rest)]] = rest
        P = np.empty((n, 3), F32); fam = np.full(n, "fill", object); sub = np.full(n, "behind", object)
        expect = np.full(n, ABSENT, np.int8); pixel = np.full((n, 2), -1, np.int64); group = np.full(n, -1, np.int64)
        for i in range(n):
            k = slots[i]
            if k < 0:
                P[i] = self.world(self.ray(self.rows // 2, self.cols // 2, -1.0 - 0.001 * (i % 97)))
                continue
            cam, f, s, e, pr, pc, _, g, world = self.recs[k]
            P[i] = world if world is not None else self.world(cam)
            fam[i], sub[i], expect[i], pixel[i], group[i] = f, s, e, (pr, pc), g
        c = Case(name=self.name, camera=self.camera, guess=self.guess if isinstance(self.guess, str) else "own", rows=self.rows, cols=self.cols,
                 K=self.K, min_d=self.min_d, max_d=self.max_d, T=self.T64.astype(F32), P=P, family=fam, sub=sub, expect=expect, pixel=pixel, group=group)
        if not self.exact:
            _expect_from_float64(c)
        return c

    def world(self, cam):
        if self.exact:
            return np.asarray(cam, F64).astype(F32)
        return (self.T64[:3, :3] @ np.asarray(cam, F64) + self.T64[:3, 3]).astype(F32)


def _expect_from_float64(case):
    """ladder cases: a point whose float64 decision is clear of every edge is expected there; group losers and fillers keep what they have"""
    ok, row, col, clear = float64_decisions(case)
    for i in range(case.n):
        if case.family[i] == "fill" or case.expect[i] == ABSENT and case.group[i] >= 0:
            continue
        if not clear[i]:
            case.expect[i] = OPEN
        elif case.group[i] >= 0 and case.expect[i] == OPEN:
            continue
        else:
            case.expect[i] = PRESENT if ok[i] else ABSENT
            case.pixel[i] = (row[i], col[i])


def tie_targets(size):
    return [k + 0.5 for k in (-1, 0, 1, 7, size // 2, size - 2, size - 1)]


TIE_SPLIT = ((0, 3, 5), (1, 4), (2, 6))      # target numbers per case: no two labels of a case want the same line


def search_ties(f, c, t, seed):
    """(x, z) pairs whose fp32 value (f x + c z) * (1 / z) is t itself, the nearest attainable value below and the one above
    -> {"tie": (x, z, 0), "below": (x, z, ulps), "above": (x, z, ulps)}, x and z arrays of up to REPEAT pairs"""
    rng = np.random.default_rng(seed)
    z = np.concatenate([F32([1.0, 2.0, 4.0, 0.75, 1.5, 3.0, 1.25, 2.5, 3.5, 0.625]), rng.uniform(0.6, 4.9, SEARCH_DEPTHS - 10).astype(F32)])
    x0 = ((t - c) * z.astype(F64) / f).astype(F32)
    assert np.all(x0 != 0)
    x = ulp_step(x0[:, None], np.arange(-ULPS, ULPS + 1)[None, :])
    zz = np.broadcast_to(z[:, None], x.shape)
    v = (F32(f) * x + F32(c) * zz) * (F32(1.0) / zz)
    tt = F32(t)
    out = {}
    for kind, mask_of in (("tie", lambda: v == tt), ("below", lambda: v == v[v < tt].max()), ("above", lambda: v == v[v > tt].min())):
        m = mask_of()
        if not m.any():
            raise AssertionError(f"round_tie: no (x, z) pair reaches {kind} of {t} with f = {f}, c = {c}: widen the search")
        a, b = np.nonzero(m)
        pick = np.unique(a, return_index=True)[1][:REPEAT]             # one pair per depth, the ten round depths first
        out[kind] = (x[a[pick], b[pick]], z[a[pick]], int(ordered(v[a[0], b[0]]) - ordered(tt)))
    return out


def round_tie_cases(camera, seed=0):
    rows, cols, K = CAMERAS[camera]
    fx, fy, cx, cy = K
    cases = []
    for axis, (f, c, size, other) in (("col", (fx, cx, cols, rows)), ("row", (fy, cy, rows, cols))):
        targets = tie_targets(size)
        for part, members in enumerate(TIE_SPLIT):
            b = _Builder(f"round_tie/{camera}/{axis}{part}", camera, RANGES[0], "identity", seed + 17 * part)
            lines = {}
            for tn in members:
                t = targets[tn]; k = int(np.floor(t))
                found = search_ties(f, c, t, seed + tn)
                for kind in ("tie", "below", "above"):
                    xs, zs, u = found[kind]
                    landed = {"tie": k + 1 if t > 0 else k, "below": k, "above": k + 1}[kind]
                    sub = f"{axis}{t:g}/" + ("tie" if kind == "tie" else f"{kind}({u}ulp)")
                    for rep in range(REPEAT):
                        x, z = xs[rep % len(xs)], zs[rep % len(zs)]
                        o = lines.get(landed, 0); lines[landed] = o + 1          # the next free line of the other axis, the last one left out
                        assert o < other - 1
                        w = (o - (cy if axis == "col" else cx)) * F64(z) / (fy if axis == "col" else fx)
                        world = np.array([x, w, z] if axis == "col" else [w, x, z]).astype(F32)
                        inside = 0 <= landed < size
                        pix = ((o, landed) if axis == "col" else (landed, o)) if inside else (-1, -1)
                        b.add(None, "round_tie", sub, PRESENT if inside else ABSENT, pix, world=world)
            cases.append(b.finish())
    return cases


def round_tie_ladder_cases(camera, guess, seed=0):
    rows, cols, K = CAMERAS[camera]
    fx, fy, cx, cy = K
    cases = []
    for axis, (size, other) in (("col", (cols, rows)), ("row", (rows, cols))):
        b = _Builder(f"round_tie/{camera}/{guess}/{axis}", camera, RANGES[0], guess, seed)
        count = 0
        for t in tie_targets(size):
            for sign in (-1, 1):
                for step in LADDER:
                    v = t + sign * step
                    o = 1 + count % (other - 2); count += 1
                    z = 1.0 + 0.25 * (count % 11)
                    cam = b.ray(o, v, z) if axis == "col" else b.ray(v, o, z)
                    b.add(cam, "round_tie", f"{axis}{t:g}/{sign * step:+.1e}")
        cases.append(b.finish())
    return cases


def depth_edge_cases(camera, seed=0):
    cases = []
    for rg in RANGES:
        b = _Builder(f"depth_edge/{camera}/{rg[0]:g}-{rg[1]:g}/identity", camera, rg, "identity", seed)
        for which, edge in (("min", rg[0]), ("max", rg[1])):
            for k in range(-2, 3):
                z = ulp_step0(edge, k)
                inside = not (z < F32(rg[0]) or z > F32(rg[1])) and abs(float(z)) > 1e-30      # a zero or denormal depth has no finite pixel
                for _ in range(REPEAT):
                    r, c = b.pixel()
                    world = b.ray(r, c, F64(z)).astype(F32); world[2] = z
                    b.add(None, "depth_edge", f"{which}{k:+d}ulp", PRESENT if inside else ABSENT, (r, c) if inside else (-1, -1), world=world)
        cases.append(b.finish())
        for guess in ("small", "moderate"):
            b = _Builder(f"depth_edge/{camera}/{rg[0]:g}-{rg[1]:g}/{guess}", camera, rg, guess, seed)
            for which, edge in (("min", rg[0]), ("max", rg[1])):
                for sign in (-1, 1):
                    for step in LADDER:
                        r, c = b.pixel()
                        z = edge * (1 + sign * step) if edge > 0 else sign * step
                        b.add(b.ray(r, c, z), "depth_edge", f"{which}{sign * step:+.1e}")
            cases.append(b.finish())
    return cases


def behind_case(camera, seed=0):
    b = _Builder(f"behind/{camera}", camera, RANGES[1], "identity", seed)
    for sub, zs in (("negative", [-0.5, -1.0, -2.0, -1e-3, -1e-30, -3.0, -5.9, -6.0]), ("plus_zero", [0.0] * REPEAT), ("minus_zero", [-0.0] * REPEAT),
                    ("denormal", [1e-45, 3e-45, 1e-40, 1.1e-38, -1e-45, -1e-40, 5e-39, 2e-42])):
        for j, z in enumerate(zs):
            r, c = b.pixel()
            ref = b.ray(r, c, 1.0 + 0.1 * j)                       # a zero or denormal depth under the x, y of a point that lands
            world = np.array([ref[0], ref[1], z], F32)
            if sub == "negative":
                world = b.ray(r, c, z).astype(F32)                 # on the pixel's ray behind the camera: only the range test rejects it
            b.add(None, "behind", sub, ABSENT, world=world)
    return b.finish()


def collide_case(camera="wide", seed=0):
    b = _Builder(f"collide/{camera}", camera, RANGES[0], "identity", seed)
    n = COLLIDE_POINTS

    def group(sub, depths_of, m, indices=None):
        """m points in one pixel; depths_of(m) -> ulp offsets from the nearest depth, offset 0 (the nearest) may repeat; the winner: the lowest
        index among the nearest.  indices None: wherever the permutation puts them (then the order of the offsets is by ascending index)."""
        r, c = b.pixel()
        z0 = F32(b.rng.uniform(1.0, 3.0))
        offs = depths_of(m)
        g = b.groups; b.groups += 1
        for j in range(m):
            z = ulp_step(z0, offs[j])
            world = b.ray(r, c, F64(z)).astype(F32); world[2] = z
            b.add(None, "collide", sub, OPEN, (r, c), index=-1 if indices is None else indices[j], group=g, world=world)
        return g

    for m in GROUPS:
        group(f"equal{m}", lambda m: np.zeros(m, np.int64), m)
        group(f"near_high{m}", lambda m: np.arange(m)[::-1], m)
        group(f"near_low{m}", lambda m: np.arange(m), m)
    own = lambda i: [i, i + 256, i + 512, i + 768]      # noqa: E731  the four points of thread i of k_project<4>'s first workgroup
    group("own_thread/near_last", lambda m: np.arange(m)[::-1], 4, own(37))
    group("own_thread/equal", lambda m: np.zeros(m, np.int64), 4, own(141))
    group("one_wave/equal", lambda m: np.zeros(m, np.int64), 64, list(range(1280, 1344)))
    group("one_wave/near_high", lambda m: np.arange(m)[::-1], 64, list(range(1408, 1472)))
    group("cross_wg/near_high", lambda m: np.arange(m)[::-1], 3, [5, 1035, 2065])
    group("cross_wg/equal", lambda m: np.zeros(m, np.int64), 3, [9, 1039, 2069])
    c = b.finish(n)
    _order_groups(c)
    return c


def _order_groups(case):
    """after the permutation: a free group's depths follow its sub label in index order (near_high: the nearest at the highest index), and the
    winner of every group is marked"""
    for g in np.unique(case.group[case.group >= 0]):
        idx = np.nonzero(case.group == g)[0]                      # ascending
        sub = case.sub[idx[0]]
        z = np.sort(case.P[idx, 2])
        if sub.startswith("near_high") or sub.endswith("near_high") or sub.endswith("near_last"):
            z = z[::-1]
        r, c = case.pixel[idx[0]]
        fx, fy, cx, cy = case.K
        for i, zi in zip(idx, z):
            case.P[i] = (F32((c - cx) * F64(zi) / fx), F32((r - cy) * F64(zi) / fy), zi)
        nearest = idx[case.P[idx, 2] == case.P[idx, 2].min()]
        case.expect[idx] = ABSENT
        case.expect[nearest.min()] = PRESENT
        for i in idx:
            if case.expect[i] == ABSENT:
                case.pixel[i] = (-1, -1)


def collide_moderate_case(camera="wide", seed=0):
    b = _Builder(f"collide/{camera}/moderate", camera, RANGES[0], "moderate", seed)
    r, c = b.pixel()
    g = b.groups; b.groups += 1
    for j in range(REPEAT):                                        # the same world point: equal depths by recomputation, the lowest index wins
        b.add(b.ray(r, c, 1.75), "collide", "recomputed/equal", OPEN, (r, c), group=g)
    for step in LADDER:                                            # depths a ladder step apart in one pixel: whoever the fp32 depth says
        r2, c2 = b.pixel()
        b.add(b.ray(r2, c2, 2.0), "collide", "recomputed/ladder")
        b.add(b.ray(r2, c2, 2.0 * (1 + step)), "collide", "recomputed/ladder")
        b.add(b.ray(r2, c2, 2.0 * (1 - step)), "collide", "recomputed/ladder")
    case = b.finish()
    idx = np.nonzero(case.group == g)[0]
    case.expect[idx] = ABSENT
    case.expect[idx.min()] = PRESENT
    case.pixel[idx.min()] = (r, c)
    lad = case.sub == "recomputed/ladder"
    case.expect[lad] = OPEN
    return case


def size_transform(j):
    """a transform of the size of `small`, another one for every j"""
    v = np.array([0.03, -0.02, 0.05, 0.01, -0.015, 0.02]) * (1.0 + 0.07 * j) * np.array([1, -1, 1, -1, 1, -1]) ** j
    return A.v2t64(v)


def _size_points(b, n, near=None):
    npix = b.rows * b.cols
    for i in range(n):
        r, c = divmod(i % npix, b.cols)
        z = near if near is not None else 1.0 + 0.001 * ((i * 7919) % 1000) + 0.5 * (i // npix)
        b.add(b.ray(r, c, z), "sizes", f"n{n}", index=i, group=0)      # a group: pixels are shared from 768 points on, nothing is expected per point


def sizes_cases(camera="wide", seed=0):
    cases = []
    for j, n in enumerate(SIZES):
        b = _Builder(f"sizes/{camera}/{n}", camera, RANGES[0], size_transform(j), seed)
        _size_points(b, n)
        cases.append(b.finish(shuffle=False))
    return cases


def stale_points(case):
    """SIZES_CAPACITY points under the case's transform, every pixel covered and all nearer than the case's own: what a cloud of that capacity
    holds behind the case's points when they are uploaded over these -- a point read past the cloud's size shows in the image"""
    b = _Builder("stale", case.camera, (case.min_d, case.max_d), case.T.astype(F64), 0)
    _size_points(b, SIZES_CAPACITY, near=0.55)
    return b.finish(shuffle=False).P


def far_case(camera="wide", seed=0):
    b = _Builder(f"far/{camera}", camera, RANGES[0], "identity", seed)
    inf, nan = np.inf, np.nan
    pts = {"pixel_beyond_2^31": [(1e9, 0, 1), (-1e9, 0, 1), (0, 1e9, 1), (0, -1e9, 1), (2.5e8, 0, 1), (-2.5e8, 0, 1), (1e30, 1e30, 1), (-1e30, 1e30, 1),
                                 (3e38, 0, 0.5), (0, -3e38, 0.5)],
           "inf": [(inf, 0, 1), (-inf, 0, 1), (0, inf, 1), (0, -inf, 1), (0, 0, inf), (0, 0, -inf), (inf, inf, inf), (inf, 0, 2), (1, 1, inf)],
           "nan": [(nan, 0, 1), (0, nan, 1), (0, 0, nan), (nan, nan, nan), (nan, 0, 2), (1, nan, 3), (nan, inf, 1), (inf, 0, nan)]}
    for sub, lst in pts.items():
        for p in lst:
            b.add(None, "far", sub, ABSENT, world=np.array(p, F32))
    c = b.finish()
    c.ask_oracle = False
    return c


_CACHE = {}


def all_cases():
    """every case, built once"""
    if "all" not in _CACHE:
        cases = []
        for cam in CAMERAS:
            cases += round_tie_cases(cam)
            for guess in ("small", "moderate"):
                cases += round_tie_ladder_cases(cam, guess)
            cases += depth_edge_cases(cam)
            cases.append(behind_case(cam))
        cases.append(collide_case())
        cases.append(collide_moderate_case())
        cases += sizes_cases()
        cases.append(far_case())
        _CACHE["all"] = cases
    return _CACHE["all"]


def case_named(name):
    return next(c for c in all_cases() if c.name == name)


def batches(cases, n=9):
    """the cases in launches of n: cases of one key (image, camera, range) together, a short launch filled up with cases of its key again"""
    out = []
    keys = []
    for c in cases:
        if c.key not in keys:
            keys.append(c.key)
    for k in keys:
        grp = [c for c in cases if c.key == k]
        for s in range(0, len(grp), n):
            chunk = grp[s:s + n]
            j = 0
            while len(chunk) < n:
                chunk.append(grp[j % len(grp)]); j += 1
            out.append(chunk)
    return out


# ------------------------------------------------------------------------------------------------------------------------ reporting
def describe_difference(case, got_index, got_depth, want_index, want_depth, limit=12):
    """the family/sub labels of the points whose pixels differ, for an assertion message"""
    gi = np.asarray(got_index).reshape(case.rows, case.cols); wi = np.asarray(want_index).reshape(case.rows, case.cols)
    diff = gi != wi
    if got_depth is not None:
        diff |= bits(np.asarray(got_depth).reshape(case.rows, case.cols)) != bits(want_depth)
    lines = []
    for r, c in zip(*np.nonzero(diff)):
        g, w = int(gi[r, c]), int(wi[r, c])
        name = lambda i: case.label(i) + f"#{i}" if 0 <= i < case.n else str(i)      # noqa: E731
        dep = "" if got_depth is None else f" depth {np.asarray(got_depth).reshape(case.rows, case.cols)[r, c]!r} want {want_depth[r, c]!r}"
        lines.append(f"pixel ({r}, {c}): got {name(g)}, want {name(w)}{dep}")
    head = f"{case.name}: {len(lines)} pixels differ"
    return "\n".join([head] + lines[:limit])


def unmet_labels(case, index_image):
    """labels the image does not show as expected -> list of strings (empty = all met)"""
    flat = np.asarray(index_image).reshape(-1)
    where = {int(i): p for p, i in enumerate(flat) if i >= 0}
    out = []
    for i in range(case.n):
        if case.expect[i] == PRESENT:
            want = int(case.pixel[i][0] * case.cols + case.pixel[i][1])
            if where.get(i) != want:
                out.append(f"{case.label(i)}#{i}: expected at pixel {tuple(case.pixel[i])}, found at {where.get(i)}")
        elif case.expect[i] == ABSENT and i in where:
            out.append(f"{case.label(i)}#{i}: expected nowhere, found at {divmod(where[i], case.cols)}")
    return out


def summary(cases=None):
    """per family: points, decisions made by rounding, expectations; per variant: pixels it changes -> lines of text"""
    cases = all_cases() if cases is None else cases
    fams = {}
    for c in cases:
        f = c.name.split("/")[0]
        e = fams.setdefault(f, [0, 0, 0, 0])
        e[0] += c.n; e[1] += rounding_decisions(c); e[2] += int((c.expect != OPEN).sum()); e[3] += 1
    lines = [f"{f}: {e[3]} cases, {e[0]} points, {e[1]} decisions made by rounding, {e[2]} expectations" for f, e in fams.items()]
    for v in VARIANTS:
        fam = "collide" if v in ("tie_high", "first_wins") else None
        lines.append(f"variant {v}: {variant_count(v, cases)} pixels changed" + (" (within collide)" if fam else ""))
    return lines


def variant_count(variant, cases=None):
    cases = all_cases() if cases is None else cases
    if variant in ("tie_high", "first_wins"):
        return sum(changed_pixels(c, variant, "collide") for c in cases if c.name.startswith("collide"))
    return sum(changed_pixels(c, variant) for c in cases if c.ask_oracle)


if __name__ == "__main__":
    print("\n".join(summary()))
