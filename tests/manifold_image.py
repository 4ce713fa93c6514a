"""Inputs and numpy model of the traversability image (ManifoldVoronoiExtractor::process, pwn_tracker2/manifold_voronoi_extractor.cpp:50-127)
for tests/test_manifold_image_cpu.py and tests/test_gpu_manifold_image.py.

The model restates only the splat (:87-121): the transformed points and normals are rows of `oracle.Cloud().add(source, T)` (`transformed`).
Everything is float32 numpy in the reference's order -- product and sum rounded one by one, conversions truncating toward zero, the squared norm
compared in float64 against 0.1 -- and the per-cell rule is the reference's loop.

Two forms that must agree bit for bit: `splat_literal` (the loop, point by point, which also records the branch every point takes) and `splat`
(events sorted by cell with a stable sort, the literal walk per cell, stopping at the first obstacle).  `splat(variant=...)` gives the wrong
models of the mutation list.

Inputs: `natural` -- merge_clouds.natural_case(with_offset=True), poses relative to frame 8; `injected_case` -- clouds built point by point under
the identity (coordinates reach the splat in every bit) with every decision of the loop on both of its sides, plus seeded clouds under small
transforms."""
import functools

import numpy as np

F = np.float32
UNTOUCHED, OBSTACLE = 30000, 65535
THR = 0.64
BRANCHES = ("outside", "obstacle_skip", "below_skip", "norm_skip", "set_obstacle", "set_height")
VARIANTS = ("fused_pz", "fused_xy", "floor", "nearest", "le", "swap", "norm_first", "cloud_order", "unstable", "saturate")
EYE = np.eye(4, dtype=F)


def transformed(cloud, T):
    """points and normals (n x 3 each) of an oracle cloud under T: rows of Cloud::add's result"""
    from oracle import oracle as O
    added = O.Cloud(); added.add(cloud, np.asarray(T, F))
    a = added.arrays()
    return a["points"][:, :3].copy(), a["normals"][:, :3].copy()


def oracle_cloud(a):
    from oracle import oracle as O
    return O.Cloud.from_arrays(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])


def cloud_arrays(points, normals):
    """an uploadable cloud around n x 3 points and normals: curvature 0.01, Omega_p = I, Omega_n = 100 I"""
    n = len(points)
    P = np.zeros((n, 4), F); P[:, :3] = points; P[:, 3] = 1
    N = np.zeros((n, 4), F); N[:, :3] = normals
    op = np.zeros((n, 16), F); on = np.zeros((n, 16), F)
    for a in range(3):
        op[:, 5 * a] = 1; on[:, 5 * a] = 100
    return dict(points=P, normals=N, curvature=np.full(n, 0.01, F), omega_p=op, omega_n=on)


# ---------------------------------------------------------------------------------------------------------------- the model
def grid_constants(resolution, xs, ys):
    """cx, cy, ires (:54-56): the resolution is a float member, 1. / it a double, ires a float"""
    return int(xs * 0.5), int(ys * 0.5), F(1.0 / float(F(resolution)))


def _trunc(v, variant):
    with np.errstate(all="ignore"):
        if variant == "floor":
            return np.floor(v).astype(np.int64)
        if variant == "nearest":
            return np.rint(v).astype(np.int64)
        return np.trunc(v).astype(np.int64)


def events(P, N, resolution, xs, ys, thr=THR, variant=None):
    """per point: row x, column y, inside, pz, normal passes (:109 does not skip), bad (:113)"""
    cx, cy, ires = grid_constants(resolution, xs, ys)
    P = np.asarray(P, F); N = np.asarray(N, F)
    with np.errstate(all="ignore"):
        if variant == "fused_xy":
            fx = (np.float64(cx) + P[:, 0].astype(np.float64) * np.float64(ires)).astype(F)
            fy = (np.float64(cy) + P[:, 1].astype(np.float64) * np.float64(ires)).astype(F)
        else:
            fx = F(cx) + P[:, 0] * ires
            fy = F(cy) + P[:, 1] * ires
        x = _trunc(fx, variant if variant in ("floor", "nearest") else None)
        y = _trunc(fy, variant if variant in ("floor", "nearest") else None)
        if variant == "swap":
            x, y = y, x
        if variant == "fused_pz":
            fz = (10000.0 - 1000.0 * P[:, 2].astype(np.float64)).astype(F)
        else:
            fz = F(10000) - F(1000) * P[:, 2]
        pz = np.trunc(fz).astype(np.int64)
        sq = ((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]) + F(0)
    inside = ~((x < 0) | (x >= xs) | (y < 0) | (y >= ys))
    normal = ~(sq.astype(np.float64) < 0.1)
    bad = N[:, 2] < F(thr)
    return x, y, inside, pz, normal, bad


def _store(pz, variant):
    if variant == "saturate":
        return int(min(max(pz, 0), 65535))
    return int(pz) & 0xFFFF


def _step(s, pz, bad, variant=None):
    """:101-120 for an event whose normal passed"""
    if s == OBSTACLE:
        return s
    if (s <= pz) if variant == "le" else (s < pz):
        return s
    return OBSTACLE if bad else _store(pz, variant)


def splat_literal(clouds, resolution, xs, ys, thr=THR, image=None, variant=None):
    """the reference's loop over [(P, N), ...] -> (image uint16 [xs, ys], inside[n], branch per point per cloud (index into BRANCHES))"""
    img = np.full((xs, ys), UNTOUCHED, np.int64) if image is None else np.asarray(image).astype(np.int64).copy()
    inside_n, branches = [], []
    for P, N in clouds:
        x, y, inside, pz, normal, bad = events(P, N, resolution, xs, ys, thr)
        br = np.zeros(len(P), np.int8)
        for i in range(len(P)):
            if not inside[i]:
                continue
            s = img[x[i], y[i]]
            if variant == "norm_first" and not normal[i]:
                br[i] = 3
            elif s == OBSTACLE:
                br[i] = 1
            elif s < pz[i]:
                br[i] = 2
            elif not normal[i]:
                br[i] = 3
            elif bad[i]:
                img[x[i], y[i]] = OBSTACLE; br[i] = 4
            else:
                img[x[i], y[i]] = int(pz[i]) & 0xFFFF; br[i] = 5
        inside_n.append(int(inside.sum())); branches.append(br)
    return img.astype(np.uint16), np.array(inside_n, np.int32), branches


def splat(clouds, resolution, xs, ys, thr=THR, image=None, variant=None):
    """events of all clouds sorted by cell (stable), then the walk per cell -> (image, inside[n], events, largest run)"""
    img = (np.full(xs * ys, UNTOUCHED, np.int64) if image is None else np.asarray(image).astype(np.int64).reshape(-1).copy())
    if variant == "cloud_order":
        order = list(range(len(clouds)))[::-1]
    else:
        order = list(range(len(clouds)))
    inside_n = np.zeros(len(clouds), np.int32)
    cells, pzs, bads = [], [], []
    for k in order:
        P, N = clouds[k]
        x, y, inside, pz, normal, bad = events(P, N, resolution, xs, ys, thr, variant)
        inside_n[k] = int(inside.sum())
        keep = inside & normal
        cells.append((x * ys + y)[keep]); pzs.append(pz[keep]); bads.append(bad[keep])
    cell = np.concatenate(cells) if cells else np.zeros(0, np.int64)
    pz = np.concatenate(pzs) if pzs else np.zeros(0, np.int64)
    bad = np.concatenate(bads) if bads else np.zeros(0, bool)
    perm = np.argsort(cell, kind="stable")
    cell, pz, bad = cell[perm], pz[perm], bad[perm]
    starts = np.nonzero(np.r_[True, cell[1:] != cell[:-1]])[0] if len(cell) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(cell)] if len(cell) else starts
    longest = int((ends - starts).max()) if len(starts) else 0
    for a, b in zip(starts, ends):
        c = cell[a]
        s = int(img[c])
        rng = range(b - 1, a - 1, -1) if variant == "unstable" else range(a, b)
        for j in rng:
            if s == OBSTACLE:
                break
            s = _step(s, int(pz[j]), bool(bad[j]), variant)
        img[c] = s
    return img.reshape(xs, ys).astype(np.uint16), inside_n, len(cell), longest


# ------------------------------------------------------------------------------------------- the kernel's walk of a cell's run
INF = 1 << 40


def walk_literal(s, pz, bad):
    for p, b in zip(pz, bad):
        s = _step(s, int(p), bool(b))
    return s


def monoid_of(pz, bad):
    """the state function of one event with 0 <= pz <= 65534 as (T, M): s >= T gives obstacle, else min(s, M)"""
    return (int(pz), INF) if bad else (INF, int(pz))


def monoid_compose(f, g):
    """f first, then g"""
    (t1, m1), (t2, m2) = f, g
    return (min(t1, t2) if m1 >= t2 else t1, min(m1, m2))


def monoid_apply(f, s):
    return OBSTACLE if (s == OBSTACLE or s >= f[0]) else min(s, f[1])


def walk_trips(s, pz, bad, width=64):
    """k_manifold_cells: the run in trips of `width` events.  A trip without a wrapped height: the state before event j is the minimum of the
    state before the trip and the trip's earlier good heights; any bad event at or below its minimum makes the obstacle; else the minimum of
    all.  A trip with a wrapped height is walked event by event."""
    pz = np.asarray(pz, np.int64); bad = np.asarray(bad, bool)
    for a in range(0, len(pz), width):
        if s == OBSTACLE:
            break
        p, b = pz[a:a + width], bad[a:a + width]
        if ((p < 0) | (p > 65534)).any():
            s = walk_literal(s, p, b)
            continue
        good = np.where(b, INF, p)
        incl = np.minimum.accumulate(good)
        before = np.minimum(s, np.r_[INF, incl[:-1]])
        s = OBSTACLE if (b & (p <= before)).any() else int(min(s, incl[-1]))
    return s


# ------------------------------------------------------------------------------------------------------------ natural input
def relative_transforms(poses, to):
    """inT * cn->transform() in double, cast to float (:66, :81-84)"""
    inv = np.linalg.inv(np.asarray(poses[to], np.float64))
    return [(inv @ np.asarray(p, np.float64)).astype(F) for p in poses]


@functools.lru_cache(maxsize=None)
def natural():
    """nine 60 x 80 room frames under the sensor mounting (robot frame, z up), poses relative to frame 8 -> (case, transforms, [(P, N)])"""
    import merge_clouds as MC
    case = MC.natural_case(with_offset=True)
    trs = relative_transforms(case["poses"], 8)
    return case, trs, [transformed(c, T) for c, T in zip(case["clouds"], trs)]


# ----------------------------------------------------------------------------------------------------------- injected input
def _ulps(x, k):
    v = F(x)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf), dtype=F)
    return v


def _neighbours(x, radius):
    """the floats within `radius` ulps of x, ascending"""
    b = np.array([x], F).view(np.int32)[0]
    i = np.arange(-radius, radius + 1, dtype=np.int64) * (1 if x >= 0 else -1) + int(b)
    return np.sort(i.astype(np.int32).view(F))


def coordinate_for(k, c, ires, frac=0.7):
    """a float p with (int)(c + p * ires) == k, about `frac` into the cell"""
    p = F((k + frac - c) / float(ires))
    assert int(np.trunc(F(c) + p * ires)) == k, (k, c, ires)
    return p


def coordinate_for_sum(k, d, c, ires):
    """a float p with c + p * ires == k + d steps, a step being the spacing of the floats at the larger of k and c (what the sum can resolve), or the nearest
    sum on that side of k where the product has no float for it"""
    step = float(np.spacing(F(max(abs(k), c, 1))))
    target = F(k + d * step)
    cand = _neighbours(F((float(target) - c) / float(ires)), 256)
    total = F(c) + cand * ires
    hit = np.nonzero(total == target)[0]
    if len(hit):
        return cand[hit[len(hit) // 2]]
    side = np.nonzero(np.sign(total - F(k)) == np.sign(d))[0]          # the product cannot reach it: the nearest sum on the same side of k
    assert len(side), (k, d, c, ires)
    return cand[side[np.argmin(np.abs(total[side].astype(np.float64) - float(target)))]]


def z_for_pz(pz):
    """a float z with (int)(10000 - 1000 z) == pz"""
    z = F((10000.0 - (pz + (0.5 if pz >= 0 else -0.5))) / 1000.0)
    assert int(np.trunc(F(10000) - F(1000) * z)) == pz, pz
    return z


def fused_xy_operands(c, ires, size, count):
    """(p, cell, fused cell) whose separately rounded c + p * ires truncates to another integer than the singly rounded one"""
    out = []
    for k in range(3, size - 2):
        if k == c:
            continue
        p = _neighbours(F((k - c) / float(ires)), 4000)
        a = np.trunc(F(c) + p * ires); b = np.trunc((np.float64(c) + p.astype(np.float64) * np.float64(ires)).astype(F))
        hit = np.nonzero((a != b) & (a >= 0) & (a < size) & (b >= 0) & (b < size))[0]
        if len(hit):
            out.append((p[hit[0]], int(a[hit[0]]), int(b[hit[0]])))
        if len(out) >= count:
            break
    return out


def fused_z_operands(count):
    out = []
    for pz in range(8000, 9400, 7):
        z = _neighbours(F((10000.0 - pz) / 1000.0), 4000)
        a = np.trunc(F(10000) - F(1000) * z); b = np.trunc((10000.0 - 1000.0 * z.astype(np.float64)).astype(F))
        hit = np.nonzero(a != b)[0]
        if len(hit):
            out.append(z[hit[0]])
        if len(out) >= count:
            break
    return out


def normal_with_squared_norm(t):
    """(nx, ny, 0) whose squared norm, as the splat sums it, is the float t in every bit: one component where a float squares to t, two (x and y,
    whose sum has one order) where none does"""
    t = F(t)
    if t == 0:
        return (F(0), F(0), F(0))
    a = _neighbours(F(np.sqrt(float(t))), 64)
    hit = np.nonzero(a * a == t)[0]
    if len(hit):
        return (a[hit[0]], F(0), F(0))
    for a0 in a[a * a < t][::-1]:
        r = float(t) - float(a0 * a0)
        b = _neighbours(F(np.sqrt(r)), 4096)
        hit = np.nonzero((a0 * a0 + b * b) + F(0) == t)[0]
        if len(hit):
            return (a0, b[hit[0]], F(0))
    raise AssertionError("no normal with squared norm %r" % t)


SIZES = (1, 63, 64, 65, 2048, 2049, 4097)      # of the seeded clouds, cyclically
REPEAT = 8
GOOD, BAD = (F(0), F(0), F(1)), (F(0), F(0), F(-1))


class _Builder:
    def __init__(self, xs, ys, resolution, n, seed):
        self.xs, self.ys, self.n = xs, ys, n
        self.cx, self.cy, self.ires = grid_constants(resolution, xs, ys)
        self.rng = np.random.default_rng(seed + 1000 * xs + ys)
        self.pts = [[] for _ in range(n)]; self.nrm = [[] for _ in range(n)]
        self.labels = []                       # (cloud, index, label, expected branch or None)
        # rows / columns 0, 1, size - 2 and size - 1 belong to the edge labels; every other label gets interior cells, each once while they last
        interior = [(r, c) for r in range(2, xs - 2) for c in range(2, ys - 2)]
        self.rng.shuffle(interior)
        self.free = interior
        self.exact = True                      # False once a cell had to be handed out twice: the expectations then only populate
        self.height = 0

    def cell(self):
        if self.free:
            return self.free.pop()
        self.exact = False
        return (int(self.rng.integers(0, self.xs)), int(self.rng.integers(0, self.ys)))

    def line(self, axis, k, kf):
        """a coordinate o on the other axis with the cells (k, o) and (kf, o) -- (o, k) and (o, kf) for axis 1 -- both free; they are taken"""
        pair = (lambda o: ((k, o), (kf, o))) if axis == 0 else (lambda o: ((o, k), (o, kf)))
        free = set(self.free)
        for o in range(2, (self.ys if axis == 0 else self.xs) - 2):
            if all(c in free for c in pair(o)):
                self.free = [c for c in self.free if c not in pair(o)]
                return o
        self.exact = False
        return 0

    def next_z(self):
        """a height above every generic point so far: a good point there is stored wherever it lands"""
        self.height += 1
        return z_for_pz(9500 - self.height)

    def xy(self, cell):
        r = min(max(cell[0], 0), self.xs - 1); c = min(max(cell[1], 0), self.ys - 1)
        return coordinate_for(r, self.cx, self.ires), coordinate_for(c, self.cy, self.ires)

    def add(self, cloud, x, y, z, normal, label, expect):
        cloud = min(cloud, self.n - 1)
        self.pts[cloud].append((x, y, z)); self.nrm[cloud].append(normal)
        self.labels.append((cloud, len(self.pts[cloud]) - 1, label, expect))

    def at(self, cloud, cell, pz, normal, label, expect):
        x, y = self.xy(cell)
        self.add(cloud, x, y, z_for_pz(pz), normal, label, expect)


def injected_case(xs=37, ys=53, resolution=0.2, n=31, seed=0):
    """n clouds for an xs x ys grid.  Cloud 0 (and cloud 1 for what needs an earlier cloud) carries the labels under the identity, at least
    REPEAT points each where the grid holds them, on a fresh cell and on a filled one; clouds 2.. are seeded clouds of SIZES points under small
    transforms, all below the labels' heights (they fill the free cells and leave the labelled ones as the labels left them), each with one event on the cell all clouds share.  -> dict(arrays per cloud, transforms, labels, exact, resolution, xs, ys)
    labels: (cloud, index, label, expected branch) -- the expectation holds when `exact` (no cell had to be shared)."""
    b = _Builder(xs, ys, resolution, n, seed)
    cx, cy, ires = b.cx, b.cy, b.ires
    tail = []                                   # what goes to the end of cloud 0: (cell, pz, normal, label, expect)
    # ---- order: the bad point blocked by a good one >= 2 049 indices earlier comes first, its bad half last
    for _ in range(REPEAT):
        c = b.cell()
        b.at(0, c, 9000, GOOD, "order/far_good", "set_height")
        tail.append((c, 9200, BAD, "order/far_bad", "below_skip"))
    # ---- xy_edge: the sum at k and 1 to 2 steps either side, k = 0, 1, size - 1, size; sums inside (-1, 0); both axes
    for axis, size, c0 in ((0, xs, cx), (1, ys, cy)):
        osize, oc = (ys, cy) if axis == 0 else (xs, cx)        # the other coordinate walks along the edge
        j = 0
        for k in (0, 1, size - 1, size):
            for d in (-2, -1, 0, 1, 2):
                for rep in range(2):
                    p = coordinate_for_sum(k, d, c0, ires)
                    got = int(np.trunc(F(c0) + p * ires))
                    q = coordinate_for(j % osize, oc, ires); j += 1
                    xyz = (p, q) if axis == 0 else (q, p)
                    b.add(0, xyz[0], xyz[1], b.next_z(), GOOD, "xy_edge/%d/%d%+d" % (axis, k, d), "set_height" if 0 <= got < size else "outside")
        for f in np.linspace(-0.95, -0.05, REPEAT):
            p = F((f - c0) / float(ires))
            assert -1 < float(F(c0) + p * ires) < 0
            q = coordinate_for(j % osize, oc, ires); j += 1
            xyz = (p, q) if axis == 0 else (q, p)
            b.add(0, xyz[0], xyz[1], b.next_z(), GOOD, "xy_edge/%d/negative" % axis, "set_height")
    # ---- fused_xy / fused_z: operands whose fused evaluation truncates to another integer
    for axis, size, c0 in ((0, xs, cx), (1, ys, cy)):
        for p, k, kf in fused_xy_operands(c0, ires, size, REPEAT):
            o = b.line(axis, k, kf)             # a row / column where neither the cell nor the fused evaluation's cell is taken
            q = coordinate_for(o, cy if axis == 0 else cx, ires)
            xyz = (p, q) if axis == 0 else (q, p)
            b.add(0, xyz[0], xyz[1], b.next_z(), GOOD, "fused_xy/%d" % axis, "set_height")
    for z in fused_z_operands(REPEAT):
        x, y = b.xy(b.cell())
        b.add(0, x, y, z, GOOD, "fused_z", "set_height")
    # ---- height_tie
    for _ in range(REPEAT):
        c = b.cell(); b.at(0, c, 9000, GOOD, "fill", "set_height"); b.at(0, c, 9000, GOOD, "height_tie/good", "set_height")
        c = b.cell(); b.at(0, c, 9000, GOOD, "fill", "set_height"); b.at(0, c, 9000, BAD, "height_tie/bad", "set_obstacle")
        c = b.cell(); b.at(0, c, 9000, GOOD, "fill", "set_height"); b.at(0, c, 9001, GOOD, "height_tie/plus1", "below_skip")
        c = b.cell(); b.at(0, c, 30000, GOOD, "height_tie/fresh", "set_height")
        c = b.cell(); b.at(0, c, 30000, BAD, "height_tie/fresh_bad", "set_obstacle")
    # ---- order
    for _ in range(REPEAT):
        c = b.cell(); b.at(0, c, 9000, BAD, "order/bad_first", "set_obstacle"); b.at(0, c, 8800, GOOD, "order/then_higher_good", "obstacle_skip")
        c = b.cell(); b.at(0, c, 9000, GOOD, "order/good_first", "set_height"); b.at(0, c, 9200, BAD, "order/then_lower_bad", "below_skip")
        c = b.cell(); b.at(0, c, 9000, GOOD, "order/good_first", "set_height"); b.at(0, c, 8800, BAD, "order/then_higher_bad", "set_obstacle")
        c = b.cell(); b.at(0, c, 9000, GOOD, "order/earlier_cloud_good", "set_height")
        b.at(1, c, 9200, BAD, "order/later_cloud_bad", "below_skip" if n > 1 else None)
    # ---- normal: squared norms around 0.1 (bad points: n.z = 0), n.z around the threshold, negative
    tenth = F(0.1)
    for name, t in (("zero", F(0)), ("0.05", F(0.05)), ("tenth-2", _ulps(tenth, -2)), ("tenth-1", _ulps(tenth, -1)), ("tenth", tenth), ("tenth+1", _ulps(tenth, 1)),
                    ("tenth+2", _ulps(tenth, 2))):
        nv = normal_with_squared_norm(t)
        for fill in (False, True):
            for _ in range(REPEAT // 2):
                c = b.cell()
                if fill:
                    b.at(0, c, 9000, GOOD, "fill", "set_height")
                b.at(0, c, 8900, nv, "normal/sq_%s" % name, "norm_skip" if float(t) < 0.1 else "set_obstacle")
    for d in (-2, -1, 0, 1, 2):
        nz = _ulps(F(THR), d)
        for fill in (False, True):
            for _ in range(REPEAT // 2):
                c = b.cell()
                if fill:
                    b.at(0, c, 9000, GOOD, "fill", "set_height")
                b.at(0, c, 8900, (F(0), F(0), nz), "normal/nz%+d" % d, "set_obstacle" if nz < F(THR) else "set_height")
    for _ in range(REPEAT):
        b.at(0, b.cell(), 8900, (F(0.1), F(0), F(-0.9)), "normal/negative", "set_obstacle")
    # ---- wrap
    for pz, name in ((-1, "minus1"), (-100, "minus100"), (-70000, "below-65536"), (30001, "30001"), (70000, "above65535")):
        for fill in (False, True):
            for rep in range(REPEAT):
                c = b.cell()
                if fill:
                    b.at(0, c, 9000, GOOD, "fill", "set_height")
                skipped = pz > (9000 if fill else UNTOUCHED)
                b.at(0, c, pz, GOOD, "wrap/%s/%s" % (name, "filled" if fill else "fresh"), "below_skip" if skipped else "set_height")
                if rep % 2 == 0 and not skipped:       # a lower point afterwards: blocked by the wrapped -1, stored over the others
                    b.at(0, c, 9100, GOOD, "wrap/after_%s" % name, "obstacle_skip" if pz == -1 else "set_height")
    # ---- crowd: >= 5 000 events of one cloud on one cell (heights falling and rising, bad ones that lie below, one that does not at the end)
    c = b.cell()
    x, y = b.xy(c)
    crowd_pz = b.rng.integers(8000, 9400, 5200)
    crowd_bad = b.rng.random(5200) < 0.3
    lo = UNTOUCHED
    for k in range(5200):
        pz = int(crowd_pz[k]); bad = bool(crowd_bad[k])
        if k in (3000, 4100):                                  # a wrapped height deep in the run: stored as 65436, lower points follow
            b.add(0, x, y, z_for_pz(-100), GOOD, "crowd/one_cloud_wrap", "set_height")
            lo = 65436
            continue
        if bad and pz <= lo:
            pz = lo + 1 + int(b.rng.integers(0, 50))          # a bad point below the height so far
        expect = "below_skip" if pz > lo else "set_height"
        if not bad and pz <= lo:
            lo = pz
        b.add(0, x, y, z_for_pz(pz), BAD if bad else GOOD, "crowd/one_cloud", expect)
    b.add(0, x, y, z_for_pz(lo - 1), BAD, "crowd/one_cloud_last", "set_obstacle")
    for cell, pz, nv, label, expect in tail:
        b.at(0, cell, pz, nv, label, expect)
    # ---- seeded clouds 2.., and the cell every cloud has an event on
    shared = b.cell()
    sx, sy = b.xy(shared)
    arrays, transforms = [], []
    from g2o_frontend_amd import synth
    half_x, half_y = xs / float(ires) * 0.6, ys / float(ires) * 0.6
    for k in range(n):
        T = EYE.copy()
        if k >= 2:
            m = SIZES[(k - 2) % len(SIZES)] - 1          # + the point on the shared cell
            T = synth.v2t(np.array([0.03 * k, -0.02 * k, 0.01 * k, 0.001 * k, -0.001 * k, 0.02 * k])).astype(F)
            P = np.stack([b.rng.uniform(-half_x, half_x, m), b.rng.uniform(-half_y, half_y, m), b.rng.uniform(-3.0, -0.5, m)], 1).astype(F)
            N = b.rng.standard_normal((m, 3)) * 0.5 + np.array([0, 0, 0.8])
            N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
            N[b.rng.random(m) < 0.1] = 0
            N[b.rng.random(m) < 0.1] *= F(0.3)
            for p, nv in zip(P, N):
                b.add(k, p[0], p[1], p[2], tuple(nv), "seeded", None)
        # the shared cell: cloud k's point, given in cloud k's own frame
        inv = np.linalg.inv(T.astype(np.float64))
        q = inv @ np.array([float(sx), float(sy), float(z_for_pz(9300 - 3 * k)), 1.0])
        nq = inv[:3, :3] @ (np.array([0, 0, 1.0]) if k % 5 else np.array([0.8, 0, 0.6]))
        b.add(k, F(q[0]), F(q[1]), F(q[2]), tuple(nq.astype(F)), "crowd/every_cloud", None)
        transforms.append(T)
    for k in range(n):
        arrays.append(cloud_arrays(np.array(b.pts[k], F).reshape(-1, 3), np.array(b.nrm[k], F).reshape(-1, 3)))
    return dict(arrays=arrays, transforms=transforms, labels=b.labels, exact=b.exact, resolution=resolution, xs=xs, ys=ys, n=n)


@functools.lru_cache(maxsize=None)
def injected(xs=37, ys=53, resolution=0.2, n=31):
    """the case, its oracle clouds and their transformed rows, made once"""
    case = injected_case(xs, ys, resolution, n)
    clouds = [oracle_cloud(a) for a in case["arrays"]]
    rows = [transformed(c, T) if len(a["points"]) else (np.zeros((0, 3), F), np.zeros((0, 3), F)) for c, T, a in zip(clouds, case["transforms"], case["arrays"])]
    return case, rows
