"""Injected inputs and models of the scene-maintenance stage (Cloud::add / transformInPlace, Merger::merge, VoxelCalculator::compute:
pwn_core/{cloud.cpp:145-186, merger.cpp:15-119, voxelcalculator.cpp:15-73}, basemath/gaussian.h) for tests/test_scene_clouds_cpu.py and
tests/test_gpu_scene_clouds.py.

Camera: 48 x 64 pixels under the identity pose, so that a point's projected depth is its z in every bit; points are placed at chosen (pixel,
depth) and `check_placement` asserts through oracle.project that each one landed in its pixel.  Gaussians are injected (oracle:
Cloud.set_gaussian_arrays; device: Cloud.debugSetGaussians): symmetric positive definite covariances of bounded condition number, means that
differ from the points, every flag word; a field its flag does not declare valid holds a recognisable filler that nothing may read.

Models.  Merger::merge: `_collapsedIndices` expected by construction -- `expected_collapsed` restates only the decision rule on the
construction's own (pixel, depth, normal) records, in float32 where a threshold decides; the fused means in float64 (`fused_means64`).
Cloud::add: R C R^t and R mu + t in float64 (`added_moments64`).  VoxelCalculator: integer keys and np.unique (`voxel_model`)."""
import functools

import numpy as np

from merge_clouds import bits, DEFAULT_STATS      # noqa: F401  (bits: -0.0 folded onto +0.0, one NaN pattern)

F = np.float32
ROWS, COLS = 48, 64
K_TINY = (50.0, 50.0, 31.5, 23.5)
EYE = np.eye(4, dtype=F)
CLOUD_KEYS = ("points", "normals", "curvature", "omega_p", "omega_n")
GAUSS_KEYS = ("mean", "cov", "info_vec", "info", "flags")
FILL_MOMENTS, FILL_INFO = F(12345.0), F(54321.0)      # what a field holds that its flag does not declare valid
# the merger's parameters: the projector's range around the merger's own depth bound (CFG) or inside it (CFG_FAR: the range's far end decides)
DIST_THR = F(0.1)
NORMAL_THR = F(np.cos(F(10 * np.pi / 180.0)))          # merger.cpp:6-8
CFG = dict(min_distance=F(0.05), max_distance=F(5.0), max_point_depth=F(4.0))
CFG_FAR = dict(CFG, max_point_depth=F(10.0))


def ulps(x, k):
    v = F(x)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf), dtype=F)
    return v


def isometry(v6):
    """a float32 isometry from (translation, rotation vector), orthonormal to rounding"""
    t, w = np.asarray(v6[:3], np.float64), np.asarray(v6[3:], np.float64)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / (th if th else 1.0)
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T.astype(F)


T_A = isometry((0.3, -0.2, 0.1, 0.2, -0.1, 0.3))
T_B = isometry((-0.05, 0.4, 0.02, -1.1, 0.7, 0.2))
T_FILL = isometry((0.0, 0.0, 0.002, 0.0, 0.0, 0.001))      # hardly a move: what it appends stays in its pixels, 2 mm behind


# ------------------------------------------------------------------------------------------------------------ arrays of a cloud
def place(rng, r, c, z, jitter=0.3):
    """points on the rays through the pixels (r, c) at depths z, up to `jitter` pixel off the centre"""
    fx, fy, cx, cy = K_TINY
    r, c = np.asarray(r, np.float64), np.asarray(c, np.float64)
    z = np.asarray(z, F); n = len(z)
    u = c + rng.uniform(-jitter, jitter, n); v = r + rng.uniform(-jitter, jitter, n)
    p = np.zeros((n, 4), F)
    p[:, 0] = ((u - cx) / fx * z.astype(np.float64)).astype(F); p[:, 1] = ((v - cy) / fy * z.astype(np.float64)).astype(F); p[:, 2] = z; p[:, 3] = 1
    return p


def cloud_arrays(rng, pts, normals=None):
    """arbitrary finite normals (unit, around -z), curvatures, exactly symmetric Omega_p, explicit symmetric Omega_n"""
    n = len(pts)
    nrm = np.zeros((n, 4), F)
    if normals is None:
        v3 = rng.standard_normal((n, 3)) * 0.02 + np.array([0, 0, -1.0])
        nrm[:, :3] = (v3 / np.linalg.norm(v3, axis=1, keepdims=True)).astype(F)
    else:
        nrm[:, :3] = normals
    curv = rng.uniform(0, 0.05, n).astype(F)
    op = np.zeros((n, 16), F); on = np.zeros((n, 16), F)
    for dst, scale in ((op, 30.0), (on, 100.0)):
        A = rng.standard_normal((n, 3, 3))
        S = ((A @ A.transpose(0, 2, 1) + np.eye(3)) * scale).astype(F)
        S = np.triu(S) + np.triu(S, 1).transpose(0, 2, 1)                      # exactly symmetric
        for a in range(3):
            for b in range(3):
                dst[:, a + 4 * b] = S[:, a, b]
    return dict(points=np.array(pts, F), normals=nrm, curvature=curv, omega_p=op, omega_n=on)


def spd(rng, n, cond, scale=1e-4):
    """n symmetric positive definite 3x3 (float64) with condition number `cond` at the most"""
    Q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    lam = scale * cond ** rng.uniform(0, 1, (n, 3))
    lam[:, 0] = scale; lam[: n // 2, 1] = scale * cond                      # half of them at the bound itself
    C = Q @ (lam[:, :, None] * Q.transpose(0, 2, 1))
    return (C + C.transpose(0, 2, 1)) / 2


def gaussians(rng, centres, flags, cond=1e3, spread=0.004):
    """Gaussian records around `centres` (n x 3) with the given flag words; column-major 3x3 blocks (symmetric: the same either way)"""
    n = len(flags)
    flags = np.asarray(flags, np.int32)
    mean = (np.asarray(centres, np.float64)[:, :3] + rng.uniform(-spread, spread, (n, 3))).astype(F)
    cov = spd(rng, n, cond).astype(F)
    cov = np.triu(cov) + np.triu(cov, 1).transpose(0, 2, 1)
    info64 = np.linalg.inv(cov.astype(np.float64))
    info = info64.astype(F); info = np.triu(info) + np.triu(info, 1).transpose(0, 2, 1)
    iv = np.einsum("nij,nj->ni", info.astype(np.float64), mean.astype(np.float64)).astype(F)
    g = dict(mean=mean, cov=cov.reshape(n, 9), info_vec=iv, info=info.reshape(n, 9), flags=flags)
    nom, noi = (flags & 1) == 0, (flags & 2) == 0
    g["mean"][nom] = FILL_MOMENTS; g["cov"][nom] = FILL_MOMENTS; g["info_vec"][noi] = FILL_INFO; g["info"][noi] = FILL_INFO
    return g


def tail_gaussians(k, start):
    """k recognisable records past the cloud's size (flags 1)"""
    i = np.arange(k, dtype=np.float64)[:, None] + start
    cov = np.tile((np.eye(3) * 0.5).reshape(1, 9), (k, 1)).astype(F)
    return dict(mean=(9000.0 + i + np.array([[0.0, 0.25, 0.5]])).astype(F), cov=cov, info_vec=np.full((k, 3), FILL_INFO, F), info=np.full((k, 9), FILL_INFO, F),
                flags=np.ones(k, np.int32))


def cat_gauss(a, b):
    return {k: np.concatenate([a[k], b[k]]) for k in GAUSS_KEYS}


def head_gauss(g, n):
    return {k: v[:n] for k, v in g.items()}


def valid_fields(g):
    """(key, rows) of every field the flags declare valid"""
    m, i = (g["flags"] & 1) != 0, (g["flags"] & 2) != 0
    return (("mean", m), ("cov", m), ("info", i), ("info_vec", i))


def check_placement(O, pts, r, c):
    """every point with a pixel (r >= 0) lands in it -- projected, under a range that holds every depth, with points of other pixels only --
    and every other point reaches no pixel"""
    pts = np.asarray(pts, F); r = np.asarray(r); c = np.asarray(c)
    inimg = np.nonzero(r >= 0)[0]
    pix = r[inimg] * COLS + c[inimg]
    order = np.argsort(pix, kind="stable")
    sp = pix[order]
    start = np.r_[0, np.nonzero(np.diff(sp))[0] + 1]
    layer = np.arange(len(sp)) - np.repeat(start, np.diff(np.r_[start, len(sp)]))
    for l in range(int(layer.max()) + 1 if len(layer) else 0):
        sel = inimg[order[layer == l]]
        idx, _ = O.project(K_TINY, EYE, 1e-3, 1e3, ROWS, COLS, pts[sel])
        assert np.array_equal(idx[r[sel], c[sel]], np.arange(len(sel))), "a point did not land in its pixel"
        assert (idx >= 0).sum() == len(sel)
    out = np.nonzero(r < 0)[0]
    if len(out):
        idx, _ = O.project(K_TINY, EYE, 1e-3, 1e3, ROWS, COLS, pts[out])
        assert (idx < 0).all(), "a point that should reach no pixel reached one"


# ---------------------------------------------------------------------------------------------------------------- Merger::merge
def expected_collapsed(r, c, z, normals, cfg, in_range=None):
    """_collapsedIndices from the construction's records: r < 0 = reaches no pixel.  The nearest point of a pixel (ties: the lowest index) among
    those inside the projector's range is its target; a point beyond max_point_depth stays -1; another point merges when |z - z_target| <
    DIST_THR and the normals' dot product > NORMAL_THR, both in float32 in the reference's order."""
    n = len(z)
    z = np.asarray(z, F); nrm = np.asarray(normals, F)
    ok = (r >= 0) & ~((z < cfg["min_distance"]) | (z > cfg["max_distance"]))
    out = np.full(n, -1, np.int32)
    pix = np.where(ok, r * COLS + c, -1)
    cand = np.nonzero(ok)[0]
    if not len(cand):
        return out
    order = cand[np.lexsort((cand, z[cand], pix[cand]))]                        # by pixel, then depth, then index
    first = np.r_[True, np.diff(pix[order]) != 0]
    target_of_pix = dict(zip(pix[order][first].tolist(), order[first].tolist()))
    t = np.array([target_of_pix[p] for p in pix[cand].tolist()], np.int64)
    with np.errstate(invalid="ignore"):
        near = np.abs(z[cand] - z[t]) < DIST_THR
        dot = ((nrm[cand, 0] * nrm[t, 0] + nrm[cand, 1] * nrm[t, 1]) + nrm[cand, 2] * nrm[t, 2]) + F(0) * F(0)
        merges = near & (dot > NORMAL_THR)
        deep = (z[cand] < 0) | (z[cand] > cfg["max_point_depth"])
    out[cand] = np.where(deep, -1, np.where(t == cand, cand, np.where(merges, t, -1)))
    return out


class Builder:
    """collects (pixel, depth, normal, flags, role) records; `finish` lays them out at chosen indices among fillers that reach no pixel"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.r, self.c, self.z, self.nrm, self.flags, self.tag, self.at = [], [], [], [], [], [], []
        self.free = iter(range(ROWS * COLS))

    def pixel(self):
        p = next(self.free)
        return p // COLS, p % COLS

    def add(self, r, c, z, normal=None, flags=1, tag="", at=None):
        if normal is None:
            v = self.rng.standard_normal(3) * 0.02 + np.array([0, 0, -1.0])
            normal = v / np.linalg.norm(v)
        self.r.append(r); self.c.append(c); self.z.append(F(z)); self.nrm.append(np.asarray(normal, F)); self.flags.append(flags); self.tag.append(tag)
        self.at.append(at)
        return len(self.z) - 1

    def outside(self, flags=0, tag="outside", at=None, kind=None):
        """a point that reaches no pixel: off one of the four sides, or behind the camera"""
        kind = self.rng.integers(0, 5) if kind is None else kind
        return self.add(-1 - int(kind), 0, F(self.rng.uniform(0.6, 3.0)), flags=flags, tag=tag, at=at)

    def finish(self, n=None, shuffle=True, cfg=CFG, tail=0, cond=1e3):
        """-> case.  Records with `at` keep that index, the others fill the remaining indices (shuffled); fillers up to n"""
        rng = self.rng
        m = len(self.z)
        n = m if n is None else n
        assert n >= m
        while len(self.z) < n:
            self.outside()
        fixed = {a: i for i, a in enumerate(self.at) if a is not None}
        assert len(fixed) == sum(a is not None for a in self.at) and all(0 <= a < n for a in fixed)
        rest = np.array([i for i, a in enumerate(self.at) if a is None], np.int64)
        slots = np.array([s for s in range(n) if s not in fixed], np.int64)
        if shuffle:
            rest = rng.permutation(rest)
        src = np.empty(n, np.int64)                                            # record at every index
        for a, i in fixed.items():
            src[a] = i
        src[slots] = rest
        r = np.array(self.r)[src]; c = np.array(self.c)[src]; z = np.array(self.z, F)[src]; nrm = np.stack(self.nrm)[src]
        flags = np.array(self.flags, np.int32)[src]; tag = np.array(self.tag, object)[src]
        pts = np.zeros((n, 4), F)
        img = r >= 0
        pts[img] = place(rng, r[img], c[img], z[img])
        fx, fy, cx, cy = K_TINY
        for kind, (u, v, s) in enumerate(((-9.0, 20.0, 1), (COLS + 8.0, 20.0, 1), (30.0, -7.0, 1), (30.0, ROWS + 6.0, 1), (30.0, 20.0, -1))):
            sel = r == -1 - kind                                               # left, right, above, below, behind
            zz = z[sel].astype(np.float64) * s
            pts[sel, 0] = ((u - cx) / fx * zz).astype(F); pts[sel, 1] = ((v - cy) / fy * zz).astype(F); pts[sel, 2] = zz.astype(F); pts[sel, 3] = 1
        z = pts[:, 2].copy()
        a = cloud_arrays(rng, pts, nrm)
        g = gaussians(rng, pts, flags, cond)
        if tail:
            g = cat_gauss(g, tail_gaussians(tail, n))
        expect = expected_collapsed(r, c, z, nrm, cfg)
        return dict(arrays=a, gauss=g, r=r, c=c, z=z, flags=flags, tag=tag, expect=expect, cfg=cfg, n=n)


LIST_LENGTHS = (0, 1, 2, 3, 7, 31, 64, 65, 200)
LIST_STRIDE = 257


@functools.lru_cache(maxsize=None)
def lists_case(seed=11):
    """one pixel per list length; the members of a list sit more than 256 indices apart (other blocks), on both sides of their target, in an
    order unrelated to their depths; every flag word on both sides; fillers reach no pixel and carry flags 0"""
    b = Builder(seed)
    rng = b.rng
    n = LIST_STRIDE * (max(LIST_LENGTHS) + 2) + 64
    for k, L in enumerate(LIST_LENGTHS):
        r, c = b.pixel()
        slots = rng.permutation(max(LIST_LENGTHS) + 1)[:L + 1]                # L + 1 slots of stride 257, offset by the list's number
        tslot = np.sort(slots)[(L + 1) // 2]                                   # the target in the middle: members on both sides
        zt = F(1.0 + 0.1 * k)
        b.add(r, c, zt, flags=1 + k % 3, tag="list%d/target" % L, at=int(tslot) * LIST_STRIDE + k)
        for j, s in enumerate(x for x in slots if x != tslot):
            b.add(r, c, zt + F(rng.uniform(0.001, 0.09)), flags=1 + int(rng.integers(0, 3)), tag="list%d/member" % L, at=int(s) * LIST_STRIDE + k)
    case = b.finish(n=n)
    col = case["expect"]
    for L in LIST_LENGTHS:
        t = np.nonzero(case["tag"] == "list%d/target" % L)[0]
        mem = np.nonzero(case["tag"] == "list%d/member" % L)[0]
        assert len(t) == 1 and len(mem) == L and col[t[0]] == t[0] and (col[mem] == t[0]).all()
        if L >= 2:
            assert (mem < t[0]).any() and (mem > t[0]).any() and (np.diff(np.sort(np.r_[mem, t])) > 256).all()
    assert (case["flags"][col < 0] == 0).all() and (case["flags"][col >= 0] > 0).all()
    return case


@functools.lru_cache(maxsize=None)
def one_pixel_case(n=1025, seed=12):
    """n - 1 members of one target: every point in one pixel, the target somewhere in the middle of the index range"""
    b = Builder(seed)
    r, c = 20, 30
    depths = F(1.0) + b.rng.permutation(n - 1).astype(F) * F(0.09 / n) + F(1e-4)
    for j in range(n):
        if j == n // 3:
            b.add(r, c, F(1.0), flags=3, tag="target", at=j)
        else:
            b.add(r, c, depths[j - (j > n // 3)], flags=1 + j % 3, tag="member", at=j)
    case = b.finish()
    assert (case["expect"] == n // 3).all()
    return case


def _threshold_records(b):
    """pixels around each threshold: (family, k) -> records; k = distance from the threshold in ulps of the threshold"""
    fam = {}
    ks = range(-4, 5)
    for rep in range(3):
        for k in ks:
            # |d - targetZ| against DIST_THR: targetZ in [0.1, 0.125), d = targetZ + diff exactly (both on the 2^-27 grid, the sum on 2^-26)
            diff = ulps(DIST_THR, k)
            tz = F(0.1) + F((7 * rep + 3) * 2.0 ** -20)
            for _ in range(4):
                if F(F(tz + diff) - tz) == diff:
                    break
                tz = ulps(tz, 1)
            d = F(tz + diff)
            assert F(d - tz) == diff and F(0.1) <= tz < F(0.125)
            r, c = b.pixel()
            b.add(r, c, tz, normal=(0, 0, -1), flags=1 + rep, tag="dist/target")
            fam.setdefault(("dist", k), []).append(b.add(r, c, d, normal=(0, 0, -1), flags=1 + (rep + k) % 3, tag="dist%+d" % k))
            # the normals' dot product against NORMAL_THR: (a, 0, -b) . (0, 0, -1) = b in every order of evaluation
            bb = ulps(NORMAL_THR, k)
            r, c = b.pixel()
            b.add(r, c, F(1.5), normal=(0, 0, -1), tag="dot/target")
            fam.setdefault(("dot", k), []).append(b.add(r, c, F(1.52), normal=(np.sqrt(1 - float(bb) ** 2), 0, -bb), tag="dot%+d" % k))
            for name, x in (("maxdepth", CFG["max_point_depth"]), ("min", CFG["min_distance"]), ("max", CFG["max_distance"])):
                r, c = b.pixel()
                fam.setdefault((name, k), []).append(b.add(r, c, ulps(x, k), tag="%s%+d" % (name, k), flags=1 + rep))
    return fam


@functools.lru_cache(maxsize=None)
def thresholds_case(far=False, seed=13):
    """every comparison of merger.cpp:49-76 within 4 ulp of its threshold, on both sides and at equality; far: max_point_depth beyond the
    projector's range, so that max_distance decides"""
    cfg = CFG_FAR if far else CFG
    b = Builder(seed)
    fam = _threshold_records(b)
    nrec = len(b.z)
    case = b.finish(cfg=cfg, shuffle=False)
    col, z = case["expect"], case["z"]
    cover = {}
    for (name, k), idx in fam.items():
        idx = np.array(idx)
        side = "below" if k < 0 else ("above" if k > 0 else "equal")
        if name == "dist":
            want = np.where(k < 0, idx - 1, -1)                                 # strictly below the threshold merges into the record before it
        elif name == "dot":
            want = np.where(k > 0, idx - 1, -1)
        elif name == "maxdepth":
            want = np.where(k <= 0, idx, -1) if not far else idx
        elif name == "min":
            want = np.where(k >= 0, idx, -1)
        else:
            want = np.where(k <= 0, idx, -1) if far else np.full(len(idx), -1)
        assert np.array_equal(col[idx], want), (name, k)
        cover[(name, side)] = cover.get((name, side), 0) + len(idx)
    active = [f for f in ("dist", "dot", "min", "maxdepth", "max") if not (f == "max" and not far) and not (f == "maxdepth" and far)]
    for f in active:
        assert cover[(f, "below")] >= 8 and cover[(f, "above")] >= 8 and cover[(f, "equal")] >= 1, (f, cover)
    case["cover"] = {"%s/%s" % k: v for k, v in cover.items() if k[0] in active}
    assert nrec == case["n"]
    return case


@functools.lru_cache(maxsize=None)
def ties_case(seed=14):
    """equal depths in a pixel (the lowest index wins, the others merge with difference 0), winners alone in their pixel, points off each side
    of the image / behind the camera / beyond max_point_depth, zero and NaN normals on either side"""
    b = Builder(seed)
    for rep in range(6):
        r, c = b.pixel()
        for j in range(2 + rep):
            b.add(r, c, F(1.25 + 0.125 * rep), normal=(0, 0, -1), flags=1 + (rep + j) % 3, tag="tie")
    for rep in range(12):
        r, c = b.pixel()
        b.add(r, c, F(0.7 + 0.2 * rep), flags=1 + rep % 3, tag="alone")
    for kind in range(5):
        for rep in range(3):
            b.outside(kind=kind, tag="outside%d" % kind)
    for rep in range(4):                                                       # beyond max_point_depth: the pixel's nearest and one behind it, both untouched
        r, c = b.pixel()
        b.add(r, c, F(4.2 + 0.1 * rep), flags=0, tag="deep"); b.add(r, c, F(4.25 + 0.1 * rep), flags=0, tag="deep")
    nan3, zero3 = (np.nan, 0, -1), (0, 0, 0)
    for name, bad in (("nan", nan3), ("zero", zero3)):
        for rep in range(3):
            r, c = b.pixel()                                                   # on the member's side: the member stays, and keeps flags it never uses
            b.add(r, c, F(2.0), normal=(0, 0, -1), tag=name + "/member-side/target"); b.add(r, c, F(2.01), normal=bad, tag=name + "/member-side/member")
            r, c = b.pixel()                                                   # on the target's side: the target is still its pixel's winner
            b.add(r, c, F(2.0), normal=bad, flags=2, tag=name + "/target-side/target"); b.add(r, c, F(2.01), normal=(0, 0, -1), tag=name + "/target-side/member")
    case = b.finish()
    col, tag = case["expect"], case["tag"]
    idx = np.arange(case["n"])
    for p in np.unique((case["r"] * COLS + case["c"])[tag == "tie"]):
        grp = np.nonzero((tag == "tie") & (case["r"] * COLS + case["c"] == p))[0]
        assert (col[grp] == grp.min()).all()
    assert (col[tag == "alone"] == idx[tag == "alone"]).all()
    assert (col[np.char.startswith(tag.astype(str), "outside")] == -1).all() and (col[tag == "deep"] == -1).all()
    for name in ("nan", "zero"):
        for side in ("member-side", "target-side"):
            t = tag == "%s/%s/target" % (name, side)
            assert (col[t] == idx[t]).all() and (col[tag == "%s/%s/member" % (name, side)] == -1).all()
    return case


@functools.lru_cache(maxsize=None)
def flags_case(seed=15, tail=0, n=None, cond=1e3):
    """targets and members with flags 1, 2, 3 in all nine combinations (two members each), and single winners of every flag word; cond = 1e6
    is the ill-conditioned class, held against the oracle only"""
    b = Builder(seed)
    for ft in (1, 2, 3):
        for fm in (1, 2, 3):
            for rep in range(3):
                r, c = b.pixel()
                b.add(r, c, F(1.0 + 0.05 * rep), flags=ft, tag="t%d/m%d/target" % (ft, fm))
                b.add(r, c, F(1.03 + 0.05 * rep), flags=fm, tag="t%d/m%d/member" % (ft, fm)); b.add(r, c, F(1.06 + 0.05 * rep), flags=fm, tag="t%d/m%d/member" % (ft, fm))
        for rep in range(3):
            r, c = b.pixel()
            b.add(r, c, F(2.0), flags=ft, tag="alone%d" % ft)
    for rep in range(20):
        b.outside()
    case = b.finish(n=n, tail=tail, cond=cond)
    col, tag = case["expect"], case["tag"]
    for ft in (1, 2, 3):
        for fm in (1, 2, 3):
            assert (col[tag == "t%d/m%d/member" % (ft, fm)] >= 0).all() and (case["flags"][tag == "t%d/m%d/member" % (ft, fm)] == fm).all()
    assert (case["flags"][col < 0] == 0).all()
    return case


MERGE_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2049)


@functools.lru_cache(maxsize=None)
def sizes_case(n, every_second, seed=16):
    """n points in index order: one per pixel (nothing merges) or two per pixel, the second merging into the first"""
    b = Builder(seed + n)
    for i in range(n):
        if every_second:
            p = i // 2
            b.add(p // COLS, p % COLS, F(1.0 + 0.04 * (i % 2)), flags=1 + i % 3, tag="pair", at=i)
        else:
            b.add(i // COLS, i % COLS, F(1.0 + (i % 7) * 0.1), flags=1 + i % 3, tag="single", at=i)
    case = b.finish()
    idx = np.arange(n)
    assert np.array_equal(case["expect"], idx - (idx % 2) if every_second else idx)
    return case


# A used cloud against a fresh one (tests/test_gpu_scene_sizes.py): the stand-alone calls read their sizes from the device's word while their
# grids come from the host's bound.  JUNK_N is the smallest content that leaves a third block of 256 stale records behind a content of 257.
JUNK_N, JUNK_CAPACITY = 600, 640
USED_SIZES = (1, 255, 256, 257)          # the block boundaries of a 256-thread grid
USED_SOURCES = (1, 256, 257)


def junk_case():
    """what the used cloud held first: JUNK_N points inside the view, two per pixel, the second merging into the first"""
    case = sizes_case(JUNK_N, True, seed=41)
    assert (case["r"] >= 0).all() and (case["expect"] != np.arange(JUNK_N)).sum() == JUNK_N // 2
    return case


@functools.lru_cache(maxsize=None)
def mirrored_case(n, seed=42):
    """n points inside the view: point i < n // 2 wins pixel i and point n - 1 - i merges into it (the middle one of an odd n stands alone), so
    the members of a pair lie as far apart as the size allows: (0, 256) of n = 257 in two blocks of 256; n = 256 is one block, and there the
    pairs span its waves"""
    b = Builder(seed + n)
    for i in range(n):
        j = min(i, n - 1 - i)
        b.add(j // COLS, j % COLS, F(1.0 + 0.04 * (i > j)), flags=1 + i % 3, tag="member" if i > j else "winner", at=i)
    case = b.finish()
    idx = np.arange(n)
    assert (case["r"] >= 0).all() and np.array_equal(case["expect"], np.minimum(idx, n - 1 - idx))
    return case


def fused_means64(g, collapsed):
    """the winners' new positions: the information-weighted mean over the target and its members, float64 -> {target: mean}"""
    fl = g["flags"]
    n = len(collapsed)
    out = {}
    cov = g["cov"].astype(np.float64).reshape(-1, 3, 3); info = g["info"].astype(np.float64).reshape(-1, 3, 3)
    for t in np.nonzero(collapsed == np.arange(n))[0]:
        mem = np.r_[t, np.nonzero((collapsed == t) & (np.arange(n) != t))[0]]
        I = np.zeros((3, 3)); v = np.zeros(3)
        for i in mem:
            if fl[i] & 2:
                Ii, vi = info[i], g["info_vec"][i].astype(np.float64)
            else:
                Ii = np.linalg.inv(cov[i]); vi = Ii @ g["mean"][i].astype(np.float64)
            I += Ii; v += vi
        if len(mem) == 1 and fl[t] & 1:
            out[int(t)] = g["mean"][t].astype(np.float64)                      # moments valid, nothing added: the mean as it is
        else:
            out[int(t)] = np.linalg.solve(I, v)
    return out


def fused_error(points_after, g_before, collapsed):
    """worst relative error of the winners' positions after a merge against `fused_means64`: |p - mean|_max / |mean|_max"""
    keep = np.nonzero((collapsed < 0) | (collapsed == np.arange(len(collapsed))))[0]
    pos = {int(i): j for j, i in enumerate(keep)}
    worst = 0.0
    for t, want in fused_means64(g_before, collapsed).items():
        got = points_after[pos[t], :3].astype(np.float64)
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    return worst


# Bars of the float64 comparisons: twice the oracle's own worst relative error per class, rounded up to one significant digit (the factor
# absorbs a change of seed; the device must equal the oracle in every bit, so it shares the oracle's distance).  Measured value beside each.
BAR_FUSED = {
    "lists": 6e-6,          # measured 3.00e-6
    "one_pixel": 2e-6,      # measured 6.76e-7
    "thresholds": 8e-4,     # measured 3.88e-4 (both parameter sets)
    "ties": 2e-4,           # measured 9.17e-5
    "flags": 6e-5,          # measured 2.61e-5
    "singles": 2e-2,        # measured 5.10e-3 (sizes, nothing merges: a third of the winners come back from the information form alone)
    "pairs": 6e-4,          # measured 2.54e-4 (sizes, every second point merges)
}
BAR_ADD_MEAN = 2e-2         # measured 7.28e-3 (records whose moments come from the information form)
BAR_ADD_COV = 6e-3          # measured 2.51e-3


def fused_bar(name):
    """the bar of a Merger::merge case by its class"""
    for k in ("singles", "pairs", "thresholds"):
        if k in name:
            return BAR_FUSED[k]
    return BAR_FUSED[name]


# ------------------------------------------------------------------------------------------- Cloud::add and transformInPlace
@functools.lru_cache(maxsize=None)
def add_source(n=259, seed=21, cond=1e3):
    """n points in front of the camera with Gaussians of every flag word (n across a block edge; n - 3 = 256 Gaussians is the edge itself)"""
    rng = np.random.default_rng(seed)
    pix = rng.permutation(ROWS * COLS)[:n]
    pts = place(rng, pix // COLS, pix % COLS, rng.uniform(0.6, 3.5, n).astype(F))
    a = cloud_arrays(rng, pts)
    g = gaussians(rng, pts, 1 + rng.permutation(n) % 3, cond)
    return dict(arrays=a, gauss=g, n=n)


def moments64(g):
    """(mean, cov) of every record in float64, through the information form where the moments are not valid"""
    n = len(g["flags"])
    mean = g["mean"].astype(np.float64).copy(); cov = g["cov"].astype(np.float64).reshape(n, 3, 3).copy()
    for i in np.nonzero((g["flags"] & 1) == 0)[0]:
        cov[i] = np.linalg.inv(g["info"][i].astype(np.float64).reshape(3, 3)); mean[i] = cov[i] @ g["info_vec"][i].astype(np.float64)
    return mean, cov


def added_moments64(g, T):
    """Gaussian3fVector::transformInPlace in float64: R mu + t, R C R^t"""
    T = np.asarray(T, np.float64); R = T[:3, :3]
    mean, cov = moments64(g)
    return mean @ R.T + T[:3, 3], R @ cov @ R.T


def added_error(g_after, g_before, T):
    """worst relative errors (mean, covariance) of transformed records against `added_moments64`, over records whose flags were not 0"""
    sel = g_before["flags"] != 0
    mean, cov = added_moments64(g_before, T)
    n = len(sel)
    gm = g_after["mean"].astype(np.float64); gc = g_after["cov"].astype(np.float64).reshape(n, 3, 3)
    em = np.abs(gm - mean)[sel].max(1) / np.abs(mean)[sel].max(1)
    ec = np.abs(gc - cov)[sel].reshape(-1, 9).max(1) / np.abs(cov)[sel].reshape(-1, 9).max(1)
    return float(em.max()), float(ec.max())


# --------------------------------------------------------------------------------------------------- VoxelCalculator::compute
VOXEL_RES = 0.25               # 1 / resolution = 4 exactly: a coordinate (index + fraction) / 4 gives index + fraction in every bit
VOXEL_MAX = (1 << 20) - 1
MASK64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def voxel_model(points, res):
    """(keys n x 3, original indices of the survivors in output order): truncation like (int)(p * inverseResolution), the first point of every
    voxel, voxels in lexicographic order"""
    inv = F(1) / F(res)
    keys = (np.asarray(points, F)[:, :3] * inv).astype(np.int32)
    _, first = np.unique(keys, axis=0, return_index=True)
    return keys, first.astype(np.int32)


def splitmix64(k):
    """the hash of the voxel table (splitmix64's finaliser) -- used to CHOOSE inputs only, never to predict an output"""
    k = np.asarray(k, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(30); k *= np.uint64(0xbf58476d1ce4e5b9); k ^= k >> np.uint64(27); k *= np.uint64(0x94d049bb133111eb); k ^= k >> np.uint64(31)
    return k


def pack_keys(idx):
    """the 63-bit word of voxel indices (ix, iy, iz), each biased by 2^20 into 21 bits: integer order = lexicographic order"""
    b = (np.asarray(idx, np.int64) + (1 << 20)).astype(np.uint64)
    return (b[:, 0] << np.uint64(42)) | (b[:, 1] << np.uint64(21)) | b[:, 2]


def unpack_keys(k):
    k = np.asarray(k, np.uint64)
    m = np.uint64((1 << 21) - 1)
    return np.stack([(k >> np.uint64(42)) & m, (k >> np.uint64(21)) & m, k & m], 1).astype(np.int64) - (1 << 20)


def points_of_keys(rng, idx, res=VOXEL_RES):
    """a point inside every voxel: (index + fraction towards away-from-zero) * res, exact for res = 0.25; index 0 gets (-1, 1) * res and -0.0"""
    idx = np.asarray(idx, np.int64)
    frac = rng.integers(0, 4, idx.shape) / 4.0
    sign = np.where(idx < 0, -1.0, np.where(idx > 0, 1.0, rng.choice([-1.0, 1.0], idx.shape)))
    p = ((np.abs(idx) + frac) * sign * res).astype(F)
    p = np.where((idx == 0) & (frac == 0) & (sign < 0), F(-0.0), p)
    pts = np.ones((len(idx), 4), F); pts[:, :3] = p
    return pts


def voxel_case(rng, idx, res=VOXEL_RES, light=False):
    """arrays of a cloud whose point i lies in voxel idx[i]; the model's keys must be idx"""
    pts = points_of_keys(rng, idx, res)
    n = len(pts)
    if light:                      # large clouds: cheap arrays, every row still its own
        i = np.arange(n, dtype=F)
        nrm = np.zeros((n, 4), F); nrm[:, 2] = -1; nrm[:, 0] = i * F(2.0 ** -22)
        op = np.zeros((n, 16), F); op[:, 0] = 1 + i; op[:, 5] = 2; op[:, 10] = 3; op[:, 1] = op[:, 4] = i * F(0.5)
        on = np.zeros((n, 16), F); on[:, 0] = on[:, 5] = on[:, 10] = 100; on[:, 2] = on[:, 8] = i
        a = dict(points=pts, normals=nrm, curvature=(i * F(2.0 ** -24)).astype(F), omega_p=op, omega_n=on)
    else:
        a = cloud_arrays(rng, pts)
    keys, first = voxel_model(pts, res)
    assert np.array_equal(keys, idx), "a point did not land in its voxel"
    return dict(arrays=a, keys=keys, kept=first, res=res, n=n)


def random_keys(rng, m, lim=VOXEL_MAX):
    """m distinct voxels over the full range on every axis"""
    k = rng.integers(-lim, lim + 1, (m + 64, 3))
    k = k[np.sort(np.unique(k, axis=0, return_index=True)[1])][:m]
    assert len(k) == m
    return k


def with_repeats(rng, keys, n, first_at=()):
    """n points over the m voxels `keys`: every voxel's first occurrence in the order given, repeats of earlier voxels in between; the first
    occurrences listed in `first_at` sit at those indices (last indices of blocks)"""
    m = len(keys)
    assert n >= m
    new = np.zeros(n, bool)
    new[0] = True
    new[list(first_at)] = True
    others = np.setdiff1d(np.arange(1, n), np.array([f + d for f in first_at for d in (0, 1)], np.int64))
    new[rng.permutation(others)[:m - int(new.sum())]] = True
    assert new.sum() == m
    count = np.cumsum(new)
    which = np.where(new, count - 1, (rng.random(n) * (count - new)).astype(np.int64))
    for f in first_at:                                                         # a repeat of it right behind the block edge
        if f + 1 < n and not new[f + 1]:
            which[f + 1] = which[f]
    return keys[which], new


def byte_family(rng, byte, count):
    """voxels whose 63-bit words differ in exactly one digit byte (byte 7 holds 7 bits)"""
    base = pack_keys(random_keys(rng, 1, VOXEL_MAX // 2))[0]
    vals = rng.permutation(128 if byte == 7 else 256)[:count].astype(np.uint64)
    words = (base & ~(np.uint64(255) << np.uint64(8 * byte))) | (vals << np.uint64(8 * byte))
    idx = unpack_keys(words)
    keep = (np.abs(idx) <= VOXEL_MAX).all(1)
    return idx[keep]


@functools.lru_cache(maxsize=None)
def voxel_digits_case(seed=31):
    """indices over the full +-(2^20 - 1) on every axis, and families that differ in exactly one of the eight digit bytes"""
    rng = np.random.default_rng(seed)
    fam = [byte_family(rng, b, 40) for b in range(8)]
    idx = np.concatenate([random_keys(rng, 700)] + fam)
    idx = idx[rng.permutation(len(idx))]
    case = voxel_case(rng, idx)
    w = pack_keys(case["keys"][case["kept"]])
    case["digit_values"] = [int(len(np.unique((w >> np.uint64(8 * b)) & np.uint64(255)))) for b in range(8)]
    assert min(case["digit_values"]) >= 40 and all(len(f) >= 30 for f in fam), case["digit_values"]
    return case


def entry_ranks(words, byte):
    """where every record stands when the sort pass of digit `byte` starts: its rank under the bytes below, ties in input order (what the
    stable passes before it leave)"""
    low = words & ((np.uint64(1) << np.uint64(8 * byte)) - np.uint64(1))
    rank = np.empty(len(words), np.int64)
    rank[np.argsort(low, kind="stable")] = np.arange(len(words))
    return rank


STABILITY_GROUPS = {2: 20 * 64 + 5 + np.arange(3),        # pass 2: three neighbours inside one 64-record step
                    5: 7 + 31 * np.arange(65),             # pass 5: 65 records over the steps of the first chunk of 2048
                    7: 40 + 13 * np.arange(300)}           # pass 7: 300 records over the first two chunks


@functools.lru_cache(maxsize=None)
def voxel_stability_case(seed=32):
    """4097 distinct voxels, every point a survivor.  Planted groups share the digit of one sort pass and differ below it.  A pass sees the
    records in the order of the bytes below its digit, so a group is chosen by that rank (STABILITY_GROUPS), lower passes first -- a digit set
    for pass p does not move a rank of a pass <= p -- and the placement is asserted on the ranks of the finished keys: 3 inside one 64-record
    step (pass 2), 65 over many steps of one chunk of 2048 (pass 5), 300 over two chunks (pass 7).  groups: pass -> (size, steps, chunks)."""
    rng = np.random.default_rng(seed)
    m = 4097
    words = pack_keys(random_keys(rng, m, VOXEL_MAX // 2))
    members = {}
    for byte in sorted(STABILITY_GROUPS):
        rank = entry_ranks(words, byte)
        at = np.empty(m, np.int64); at[rank] = np.arange(m)                     # record at every rank
        mem = at[STABILITY_GROUPS[byte]]
        shift = np.uint64(8 * byte)
        d = (words[mem[0]] >> shift) & np.uint64(255)
        words[mem] = (words[mem] & ~(np.uint64(255) << shift)) | (d << shift)
        members[byte] = mem
    idx = unpack_keys(words)
    assert (np.abs(idx) <= VOXEL_MAX).all() and len(np.unique(words)) == m
    groups = {}
    for byte, mem in members.items():
        rank = entry_ranks(words, byte)[mem]
        assert np.array_equal(np.sort(rank), STABILITY_GROUPS[byte])            # later digits moved nothing below them
        assert len(np.unique((words[mem] >> np.uint64(8 * byte)) & np.uint64(255))) == 1
        assert len(np.unique(words[mem] & ((np.uint64(1) << np.uint64(8 * byte)) - np.uint64(1)))) == len(mem)      # told apart by the bytes below only
        groups[byte] = (len(mem), len(np.unique(rank // 64)), len(np.unique(rank // 2048)))
    assert groups[2] == (3, 1, 1) and groups[5][0] == 65 and groups[5][1] >= 30 and groups[5][2] == 1 and groups[7][0] == 300 and groups[7][2] == 2
    case = voxel_case(rng, idx)
    case["groups"] = groups
    assert len(case["kept"]) == m
    return case


VOXEL_SURVIVORS = (1, 2, 63, 64, 65, 2047, 2048, 2049, 4097)
VOXEL_SIZES = (1, 1023, 1024, 1025)


@functools.lru_cache(maxsize=None)
def voxel_survivors_case(m, repeats, seed=33):
    """m surviving voxels: every point its own voxel, or with repeats of earlier voxels in between (n = m + m // 2 + 1)"""
    rng = np.random.default_rng(seed + m)
    keys = random_keys(rng, m)
    idx = with_repeats(rng, keys, m + m // 2 + 1)[0] if repeats else keys
    case = voxel_case(rng, idx)
    assert len(case["kept"]) == m
    return case


@functools.lru_cache(maxsize=None)
def voxel_sizes_case(n, variant, seed=34):
    """n points: "one" voxel for all (every point contends for one table entry), "distinct", or "edges" -- repeats whose first occurrence is
    the last index of a block of 256"""
    rng = np.random.default_rng(seed + n)
    if variant == "one":
        idx = np.tile(random_keys(rng, 1), (n, 1))
    elif variant == "distinct":
        idx = random_keys(rng, n)
    else:
        edges = [e for e in (255, 511, 767, 1023) if e < n - 1]
        m = max(1, n // 2)
        idx, new = with_repeats(rng, random_keys(rng, m), n, first_at=edges)
        assert all(new[e] for e in edges)
    case = voxel_case(rng, idx)
    if variant == "one":
        assert np.array_equal(case["kept"], [0])
    return case


@functools.lru_cache(maxsize=None)
def voxel_signs_case(seed=35):
    """coordinates in (-1, 1) * resolution share voxel 0 by truncation, -0.0 included; the neighbours at exactly +-resolution do not"""
    rng = np.random.default_rng(seed)
    res = F(VOXEL_RES)
    vals = np.array([0.0, -0.0, 0.9, -0.9, 1e-30, -1e-30, 0.999999, -0.999999, 0.5, -0.5], F) * res
    pts = np.ones((len(vals) * 3 + 6, 4), F); pts[:, :3] = 0
    for a in range(3):
        pts[a * len(vals):(a + 1) * len(vals), a] = vals
        pts[3 * len(vals) + 2 * a, a] = res; pts[3 * len(vals) + 2 * a + 1, a] = -res
    pts[1, :3] = F(-0.0)
    a = cloud_arrays(rng, pts)
    keys, first = voxel_model(pts, float(res))
    assert (keys[:3 * len(vals)] == 0).all() and len(first) == 7 and np.signbit(pts[1, 0])
    return dict(arrays=a, keys=keys, kept=first, res=float(res), n=len(pts))


@functools.lru_cache(maxsize=None)
def voxel_probe_case(seed=36, n=300):
    """n <= 512 points (a table of 1024 entries): 8 voxels whose home entry is the last one and 8 whose home entry is the one before, so that
    probing wraps to entry 0; each of them twice"""
    rng = np.random.default_rng(seed)
    mask = np.uint64(1023)
    cand = random_keys(rng, 60000)
    home = splitmix64(pack_keys(cand)) & mask
    last, before = cand[home == mask][:8], cand[home == mask - np.uint64(1)][:8]
    assert len(last) >= 6 and len(before) >= 6
    assert ((splitmix64(pack_keys(last)) & mask) == mask).all() and ((splitmix64(pack_keys(before)) & mask) == mask - np.uint64(1)).all()
    planted = np.concatenate([before, last])
    other = cand[(home != mask) & (home != mask - np.uint64(1))][:n - 2 * len(planted)]
    idx = np.concatenate([planted, other, planted])
    idx = idx[rng.permutation(len(idx))]
    assert len(idx) == n <= 512
    case = voxel_case(rng, idx)
    case["planted"] = (len(last), len(before))
    return case


def voxel_bound_cases(seed=37):
    """per axis and sign: (case with |p * inverseResolution| one float below 2^20 -- accepted, sorts last / first --, the same cloud with that
    coordinate at 2^20 exactly -- refused)"""
    rng = np.random.default_rng(seed)
    out = []
    lim = F(2.0 ** 20 * VOXEL_RES)
    for axis in range(3):
        for sign in (1, -1):
            idx = random_keys(rng, 40, 1000)
            idx[:, :axis] = idx[0, :axis]                                      # the axes before it equal: this axis decides the order
            pts = points_of_keys(rng, idx)
            below = np.nextafter(lim, F(0)) * F(sign)
            pts[17, axis] = below
            a = cloud_arrays(rng, pts)
            keys, first = voxel_model(pts, VOXEL_RES)
            assert keys[17, axis] == sign * VOXEL_MAX and first[-1 if sign > 0 else 0] == 17
            bad = {k: v.copy() for k, v in a.items()}
            bad["points"][17, axis] = lim * F(sign)
            out.append((axis, sign, dict(arrays=a, keys=keys, kept=first, res=VOXEL_RES, n=40), bad))
    return out


CARRY_N = 1024 * 1024 + 1025


@functools.lru_cache(maxsize=1)
def voxel_carry_case(seed=38):
    """1024 * 1024 + 1025 points: more than 1024 block sums, so that the scan's carry crosses into its second tile; a seeded keep pattern"""
    rng = np.random.default_rng(seed)
    n = CARRY_N
    m = n // 2
    # distinct voxels without a sort of a million rows: a bijection of the voxel's number onto three 7-bit-shifted fields
    num = rng.permutation(1 << 21)[:m].astype(np.int64)
    keys = np.stack([(num & 127) * 9001 - 500000, ((num >> 7) & 127) * 7919 - 480000, (num >> 14) * 6007 - 350000], 1)
    new = np.zeros(n, bool); new[0] = True
    new[1 + rng.permutation(n - 1)[:m - 1]] = True
    count = np.cumsum(new)
    which = np.where(new, count - 1, (rng.random(n) * (count - new)).astype(np.int64))
    case = voxel_case(rng, keys[which], light=True)
    assert len(case["kept"]) == m and np.array_equal(case["kept"], np.nonzero(new)[0][np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))])
    case["new"] = new
    return case


# ------------------------------------------------------------------------------------------------------- the oracle's side
def oracle_cloud(O, arrays, gauss=None):
    c = O.Cloud.from_arrays(*[arrays[k] for k in CLOUD_KEYS])
    if gauss is not None:
        c.set_gaussian_arrays(*[gauss[k] for k in GAUSS_KEYS])
    return c


def oracle_merge(O, cloud, cfg, T=EYE):
    """Merger::merge with the thresholds of this module -> (new size, _collapsedIndices)"""
    return O.merge(cloud, K_TINY, T, float(cfg["min_distance"]), float(cfg["max_distance"]), ROWS, COLS, float(DIST_THR), float(NORMAL_THR),
                   float(cfg["max_point_depth"]))


def merge_cases():
    """(name, case) of every Merger::merge class"""
    out = [("lists", lists_case()), ("one_pixel", one_pixel_case()), ("thresholds", thresholds_case(False)), ("thresholds_far", thresholds_case(True)),
           ("ties", ties_case()), ("flags", flags_case())]
    out += [("size%d_%s" % (n, "pairs" if e else "singles"), sizes_case(n, e)) for n in MERGE_SIZES for e in (False, True)]
    return out


def voxel_cases():
    """(name, case) of every VoxelCalculator class but the bound and the carry"""
    out = [("digits", voxel_digits_case()), ("stability", voxel_stability_case()), ("signs", voxel_signs_case()), ("probe", voxel_probe_case())]
    out += [("survivors%d_%s" % (m, "repeats" if r else "distinct"), voxel_survivors_case(m, r)) for m in VOXEL_SURVIVORS for r in (False, True)]
    out += [("n%d_%s" % (n, v), voxel_sizes_case(n, v)) for n in VOXEL_SIZES for v in ("one", "distinct", "edges")]
    return out


# ------------------------------------------------------------------------- one call sequence on either side (oracle / device)
CONVERTER_CONF = dict(min_distance=0.5, max_distance=4.5, world_radius=0.1, min_image_radius=2, max_image_radius=5, min_points=8,
                      stats_curvature_threshold=0.2, point_info_curvature_threshold=0.02, normal_info_curvature_threshold=0.02)


def plane_frame():
    """a 48 x 64 depth frame of a slanted plane with a step and a hole: what the converter turns into a cloud with Stats and class-coded
    normal information"""
    r, c = np.mgrid[0:ROWS, 0:COLS]
    d = (1.2 + 0.004 * c + 0.003 * r).astype(F)
    d[30:, 40:] += F(0.35)
    d[5:9, 7:12] = 0
    return d


class OracleSide:
    name = "oracle"

    def __init__(self, O):
        self.O = O

    def cloud(self, arrays, gauss=None, capacity=None):
        return oracle_cloud(self.O, arrays, gauss)

    def empty(self, capacity):
        return self.O.Cloud()

    def converted(self, depth, keep_stats):
        c = self.O.convert(self.O.converter_params(K=K_TINY, **CONVERTER_CONF), depth)[0]
        # a device cloud converted without keep_stats carries no Stats: its points are appended with the default Stats, as an uploaded cloud's
        return c if keep_stats else oracle_cloud(self.O, c.arrays())

    def set_gaussians(self, c, g):
        c.set_gaussian_arrays(*[g[k] for k in GAUSS_KEYS])

    def stale(self, c, capacity, keep):
        if keep is not None:
            self.set_gaussians(c, keep)

    def add(self, dst, src, T):
        dst.add(src, T)

    def transform(self, c, T):
        c.transform_in_place(T)

    def merge(self, c, cfg, T=EYE):
        return oracle_merge(self.O, c, cfg, T)

    def voxelize(self, c, res):
        return self.O.voxelize(c, res, literal=False)

    def snapshot(self, c, stats=True):
        a = c.arrays(stats=stats)
        a["gauss"] = c.gaussians()
        return a


class DeviceSide:
    name = "device"

    def __init__(self, ctx):
        from g2o_frontend_amd import api
        self.api, self.ctx = api, ctx
        proj = api.PinholePointProjector()
        proj.setCameraMatrix([[K_TINY[0], 0, K_TINY[2]], [0, K_TINY[1], K_TINY[3]], [0, 0, 1]])
        proj.setMinDistance(CONVERTER_CONF["min_distance"]); proj.setMaxDistance(CONVERTER_CONF["max_distance"]); proj.setImageSize(ROWS, COLS)
        st = api.StatsCalculatorIntegralImage()
        st.setWorldRadius(CONVERTER_CONF["world_radius"]); st.setMinImageRadius(CONVERTER_CONF["min_image_radius"])
        st.setMaxImageRadius(CONVERTER_CONF["max_image_radius"]); st.setMinPoints(CONVERTER_CONF["min_points"])
        st.setCurvatureThreshold(CONVERTER_CONF["stats_curvature_threshold"])
        pi, ni = api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator()
        pi.setCurvatureThreshold(CONVERTER_CONF["point_info_curvature_threshold"]); ni.setCurvatureThreshold(CONVERTER_CONF["normal_info_curvature_threshold"])
        self.converter = api.DepthImageConverterIntegralImage(proj, st, pi, ni)
        self.voxel = api.VoxelCalculator()

    def cloud(self, arrays, gauss=None, capacity=None):
        n = len(arrays["points"])
        c = self.api.Cloud(self.ctx, max(1, n if capacity is None else capacity))
        if n:
            c.upload(*[arrays[k] for k in CLOUD_KEYS])
        if gauss is not None:
            self.set_gaussians(c, gauss)
        return c

    def empty(self, capacity):
        return self.api.Cloud(self.ctx, max(1, capacity))

    def converted(self, depth, keep_stats):
        c = self.api.Cloud(self.ctx, ROWS * COLS)
        self.converter.compute(c, depth, keep_stats=keep_stats)
        return c

    def set_gaussians(self, c, g):
        c.debugSetGaussians(*[g[k] for k in GAUSS_KEYS])

    def stale(self, c, capacity, keep):
        """junk in every record of the buffer, then the vector the cloud is meant to have (none: an empty one over the same buffer)"""
        self.set_gaussians(c, junk_gaussians(capacity))
        self.set_gaussians(c, keep if keep is not None else junk_gaussians(0))

    def add(self, dst, src, T):
        dst.add(src, T)

    def transform(self, c, T):
        c.transformInPlace(T)

    def merge(self, c, cfg, T=EYE):
        api = self.api
        proj = api.PinholePointProjector()
        proj.setCameraMatrix([[K_TINY[0], 0, K_TINY[2]], [0, K_TINY[1], K_TINY[3]], [0, 0, 1]])
        proj.setMinDistance(float(cfg["min_distance"])); proj.setMaxDistance(float(cfg["max_distance"])); proj.setImageSize(ROWS, COLS)
        m = api.Merger(); m.setImageSize(ROWS, COLS); m.setMaxPointDepth(float(cfg["max_point_depth"]))
        m.setDistanceThreshold(float(DIST_THR)); m.setNormalThreshold(float(NORMAL_THR))
        m.setDepthImageConverter(api.DepthImageConverterIntegralImage(proj, None, None, None))
        k = m.merge(c, np.asarray(T, F))
        return k, m.collapsedIndices().copy()

    def voxelize(self, c, res):
        k = self.voxel.compute(c, res)
        return k, self.voxel.keptIndices().copy()

    def snapshot(self, c, stats=True):
        a = c.arrays(stats=stats)
        a["gauss"] = c.gaussians()
        return a


def junk_gaussians(n):
    """records that must never show: both forms declared valid, every float 777"""
    return dict(mean=np.full((n, 3), 777, F), cov=np.full((n, 9), 777, F), info_vec=np.full((n, 3), 777, F), info=np.full((n, 9), 777, F),
                flags=np.full(n, 3, np.int32))


ADD_DESTINATIONS = ("empty", "points", "gaussians")
ADD_TRANSFORMS = (("identity", EYE), ("A", T_A), ("B", T_B))


def add_sequence(side, ngauss, dst_kind, T, source="uploaded"):
    """Cloud::add of a source with `ngauss` Gaussians into an empty destination / one that holds points only / one with Gaussians, then
    transformInPlace(T_B) on the result -> [snapshot after add, snapshot after the transform], the source's and destination's Gaussians before"""
    src = add_source()
    n = src["n"]
    g = head_gauss(src["gauss"], ngauss) if ngauss else None
    if source == "uploaded":                     # explicit normal information, no Stats
        s = side.cloud(src["arrays"], g)
    elif source == "added":                      # explicit normal information and Stats: a cloud a Cloud::add made
        s = side.empty(n); side.add(s, side.cloud(src["arrays"]), T_A)
        if g is not None:
            side.set_gaussians(s, g)
    else:                                        # "converted" / "converted_no_stats": class-coded normal information
        s = side.converted(plane_frame(), keep_stats=source == "converted")
        nc = len(side.snapshot(s, stats=False)["points"])
        g = gaussians(np.random.default_rng(5), np.zeros((nc, 3)), 1 + np.arange(nc) % 3, spread=2.0) if ngauss else None
        if g is not None:
            g = head_gauss(g, nc - (n - ngauss))
            side.set_gaussians(s, g)
        n = nc
    d0 = add_source(n=70, seed=22)
    if dst_kind == "empty":
        dst, gd = side.empty(2 * ROWS * COLS), None
    elif dst_kind == "points":
        dst, gd = side.cloud(d0["arrays"], None, capacity=2 * ROWS * COLS), None
    else:
        dst, gd = side.cloud(d0["arrays"], d0["gauss"], capacity=2 * ROWS * COLS), d0["gauss"]
    side.add(dst, s, T)
    snaps = [side.snapshot(dst)]
    side.transform(dst, T_B)
    snaps.append(side.snapshot(dst))
    return snaps, g, gd, n


LONG_TAIL = 5


def add_long_sequence(side, dst_kind, T):
    """Cloud::add of a source whose Gaussian vector is LONG_TAIL records longer than its points, then transformInPlace(T_B): the destination's
    vector grows by the source's count, the records past the source's points are default Gaussians (cloud.cpp:153).  The device's buffer is
    first filled with junk records up to its capacity and the vector cut back (`stale`), so that whatever the call fails to write shows.
    -> [snapshot after add, after the transform], points before, source points"""
    src = add_source()
    n = src["n"]
    g = cat_gauss(src["gauss"], tail_gaussians(LONG_TAIL, n))
    s = side.cloud(src["arrays"], g, capacity=n + LONG_TAIL)
    d0 = add_source(n=70, seed=22)
    cap = 70 + n + LONG_TAIL + 11
    if dst_kind == "empty":
        dst, k, keep = side.empty(cap), 0, None
    else:
        dst, k, keep = side.cloud(d0["arrays"], None, capacity=cap), 70, (d0["gauss"] if dst_kind == "gaussians" else None)
    side.stale(dst, cap, keep)
    side.add(dst, s, T)
    snaps = [side.snapshot(dst)]
    side.transform(dst, T_B)
    snaps.append(side.snapshot(dst))
    return snaps, k, n
