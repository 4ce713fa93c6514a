"""Inputs and numpy model of the cloud-level fusion (Merger2::merge, pwn_tracker2/merger2.cpp:106-183, called per node by
PwnMerger::mergeNodeList, pwn_tracker2/pwn_merger.cpp:28-62) for tests/test_merge_clouds_cpu.py and tests/test_gpu_merge_clouds.py.

The model does not restate Cloud::add: the arrays of an appended point are rows of `oracle.Cloud().add(source, T)`, gathered by idx_current at
the appended pixels in raster order.  For T = identity Cloud::add skips the transform (cloud.cpp:176) and Merger2::merge does not: there the
model multiplies in float32 in the reference's order itself -- the information matrices by `omega_transform` (they may hold non-finite entries,
which a product with exact zeros turns into NaN), everything else is finite and a product with the identity returns its bits (the sign of a
zero apart, which the comparisons fold).  The projections are oracle.project's, the projector matrices oracle.projector_matrices'.  The fuse
branch is float32 numpy in the reference's order: separately rounded products, one sum, one division; the comparisons against the reference's
double literals are made in float64.

Deviation kept from the kernels' side and documented in docs/parity.md: the Stats block of an appended point is T * the source point's own
block (what Cloud::add stores), not the reference's running product over every earlier append (:139-143).

Two forms that must agree bit for bit: `merge_list` (vectorised) and `merge_list_literal` (the reference's loop, pixel by pixel).

Inputs: `natural_case` -- seeded room frames along a trajectory, converted by the oracle with Stats and Gaussians; `injected_case` -- a total
and incoming clouds built pixel by pixel under identity cameras (the projected depth is the point's z in every bit), every threshold of the
loop on both of its sides."""
import functools

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
K_SMALL = (65.6, 65.6, 39.5, 29.5)              # the 60 x 80 natural case (the merged closure's)
EYE = np.eye(4, dtype=F)
CLOUD_KEYS = ("points", "normals", "curvature", "omega_p", "omega_n", "stats", "eigenvalues", "npoints")
GAUSS_KEYS = ("mean", "cov", "info_vec", "info", "flags")
WIDTH = dict(points=4, normals=4, curvature=0, omega_p=16, omega_n=16, stats=16, eigenvalues=3, npoints=0, mean=3, cov=9, info_vec=3, info=9, flags=0)
DEFAULT_STATS = np.eye(4, dtype=F).reshape(-1)   # Stats(): identity block, eigenvalues 0, n 0 (stats.h:21-27)
ACTIONS = ("append_new", "fuse", "append_occluder", "drop_unproject", "drop_between", "drop_depth")


def bits(a):
    """bit patterns with -0.0 folded onto +0.0 (the reference's 4x4 products add exact-zero fourth terms, the kernels' 3x3 products do not:
    tests/test_scene.py) and every NaN onto one pattern (x86 and the GPU give the NaN they make different signs)"""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    a = a.copy(); a[a == 0] = 0; a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def raw_bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the total
def empty_total(gauss=False):
    t = {k: np.zeros((0, WIDTH[k]) if WIDTH[k] else 0, np.int32 if k == "npoints" else F) for k in CLOUD_KEYS}
    t["weights"] = np.zeros(0, F)
    t["gauss"] = {k: np.zeros((0, WIDTH[k]) if WIDTH[k] else 0, np.int32 if k == "flags" else F) for k in GAUSS_KEYS} if gauss else None
    return t


def total_from_arrays(a, weights):
    """a total that was uploaded (no Stats: the defaults; no Gaussians)"""
    n = len(a["points"])
    t = {k: np.array(a[k], F) for k in ("points", "normals", "curvature", "omega_p", "omega_n")}
    t["stats"] = np.tile(DEFAULT_STATS, (n, 1)); t["eigenvalues"] = np.zeros((n, 3), F); t["npoints"] = np.zeros(n, np.int32)
    t["weights"] = np.array(weights, F); t["gauss"] = None
    return t


def copy_total(t):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}
    if t["gauss"] is not None:
        out["gauss"] = {k: v.copy() for k, v in t["gauss"].items()}
    return out


def same_total(a, b):
    """every array of two model totals in every bit (after `bits`' folding)"""
    if len(a["points"]) != len(b["points"]) or (a["gauss"] is None) != (b["gauss"] is None):
        return False
    ok = all(np.array_equal(bits(a[k]), bits(b[k])) for k in CLOUD_KEYS + ("weights",))
    if a["gauss"] is not None:
        ok = ok and all(np.array_equal(bits(a["gauss"][k]), bits(b["gauss"][k])) for k in GAUSS_KEYS)
    return ok


# ------------------------------------------------------------------------------------------------ what an append pushes back
def omega_transform(T, om):
    """InformationMatrix::transform (T Omega T^t on the 3x3 block) of n column-major 4x4 matrices in float32: the inner products left to
    right, each product rounded on its own -- the order of Cloud::transformInPlace (cloud.cpp:173-186)"""
    T = np.asarray(T, F); om = np.asarray(om, F)
    O = lambda r, c: om[:, r + 4 * c]      # noqa: E731
    out = om.copy()
    with np.errstate(all="ignore"):
        t1 = [[(T[a, 0] * O(0, b) + T[a, 1] * O(1, b)) + T[a, 2] * O(2, b) for b in range(3)] for a in range(3)]
        for a in range(3):
            for b in range(3):
                out[:, a + 4 * b] = (t1[a][0] * T[b, 0] + t1[a][1] * T[b, 1]) + t1[a][2] * T[b, 2]
    return out


def pushed_back(src, T, gauss):
    """the arrays Merger2::merge pushes back for every point of `src` (an oracle cloud) under `T`: Cloud::add's, without its identity shortcut
    -> (arrays incl. Stats, Gaussians or None)"""
    from oracle import oracle as O
    T = np.asarray(T, F)
    if np.array_equal(T, EYE):
        a = src.arrays(stats=True)
        for k in ("points", "normals", "stats"):
            assert np.isfinite(a[k]).all(), k          # identity * finite = the same bits (sign of zero apart)
        a["omega_p"] = omega_transform(T, a["omega_p"]); a["omega_n"] = omega_transform(T, a["omega_n"])
        g = src.gaussians() if gauss else None
        if g is not None:
            assert (g["flags"] == 1).all() and np.isfinite(g["mean"]).all() and np.isfinite(g["cov"]).all()
            g["info"][:] = 0; g["info_vec"][:] = 0     # Gaussian3f(mean, cov, false): the information form starts empty (gaussian3.h:65-73)
        return a, g
    added = O.Cloud(); added.add(src, T)
    return added.arrays(stats=True), (added.gaussians() if gauss else None)


def _append(t, a, g, idx, peso):
    for k in CLOUD_KEYS:
        t[k] = np.concatenate([t[k], a[k][idx]])
    t["weights"] = np.concatenate([t["weights"], peso.astype(F)])
    if t["gauss"] is not None:
        for k in GAUSS_KEYS:
            t["gauss"][k] = np.concatenate([t["gauss"][k], g[k][idx]])


# ---------------------------------------------------------------------------------------------------------------- the model
def _projections(t, src_points, T, proj):
    """idx_current / scaledImage_current under `offset` (:113-116); indexImage_tot / depthImage_tot under T * offset, -1 / 0 for an empty total
    (:118-127); iKRt of the second projector"""
    from oracle import oracle as O
    K, offset, mn, mx, rows, cols = proj
    if len(src_points):
        idx_c, dep_c = O.project(K, offset, mn, mx, rows, cols, src_points)
    else:
        idx_c, dep_c = np.full((rows, cols), -1, np.int32), np.full((rows, cols), FLT_MAX, F)
    Ttot = O.iso_mul(np.asarray(T, F), np.asarray(offset, F))            # Isometry3f * Isometry3f
    if len(t["points"]):
        idx_t, dep_t = O.project(K, Ttot, mn, mx, rows, cols, t["points"])
    else:
        idx_t, dep_t = np.full((rows, cols), -1, np.int32), np.zeros((rows, cols), F)
    return idx_c, dep_c, idx_t, dep_t, O.projector_matrices(K, Ttot)[1]


def merge_list(total, sources, transforms, proj, gauss=False, variant=None):
    """n successive Merger2::merge calls on a copy of `total` -> (total, appended[n], fused[n], counts[n] (dict per cloud over ACTIONS, and the action per pixel as "image"), diff).
    proj = (K, offset, min_distance, max_distance, rows, cols).  variant: None = the reference; "fma" / "rcp" / "float015" / "column_order" /
    "occluder015" = the wrong kernels of the mutation list (docs/parity.md); diff counts, over the list, the pixels the inputs tell each of
    them apart on (from the same operands as the right branch)."""
    t = copy_total(total)
    K, offset, mn, mx, rows, cols = proj
    appended, fused, counts = [], [], []
    diff = dict(fma=0, rcp=0, float015=0, column_order=0, occluder015=0)
    with np.errstate(all="ignore"):
        for src, T in zip(sources, transforms):
            a, g = pushed_back(src, T, gauss)
            idx_c, d, idx_t, dep_t, iKRt = _projections(t, src.arrays()["points"], T, proj)
            d64 = d.astype(np.float64)
            sel = (d64 > 0.2) & (d64 < 100)                                       # :131
            new = sel & (idx_t < 0)                                               # :134
            delta = d - dep_t                                                     # float32
            near64 = np.abs(delta).astype(np.float64) < .15                       # :153
            near32 = np.abs(delta) < F(.15)
            near = near32 if variant == "float015" else near64
            inrange = ~((d < F(mn)) | (d > F(mx)))                                # unProject's range test (pinholepointprojector.h:246-251)
            fuse = sel & ~new & near & inrange
            occ64 = delta.astype(np.float64) < -.3                                # :164
            occ15 = delta.astype(np.float64) < -.15
            occl = sel & ~new & ~near & (occ15 if variant == "occluder015" else occ64)
            app = new | occl
            diff["float015"] += int((sel & ~new & (near32 != near64)).sum())
            diff["occluder015"] += int((sel & ~new & ~near64 & (occ15 != occ64)).sum())
            counts.append(dict(append_new=int(new.sum()), fuse=int(fuse.sum()), append_occluder=int(occl.sum()),
                               drop_unproject=int((sel & ~new & near & ~inrange).sum()), drop_between=int((sel & ~new & ~near & ~occl).sum()),
                               drop_depth=int((~sel).sum())))
            counts[-1]["image"] = np.where(new, 0, np.where(fuse, 1, np.where(occl, 2, np.where(sel & ~new & near, 3, np.where(sel, 4, 5)))))   # index into ACTIONS
            # the fuses: every index of the total sits in at most one pixel
            rr, cc = np.nonzero(fuse)
            dd = d[rr, cc]; it = idx_t[rr, cc]
            assert len(np.unique(it)) == len(it)
            x, y = cc.astype(F) * dd, rr.astype(F) * dd
            peso = F(1) / dd
            pt = t["weights"][it]; somma = pt + peso
            for k in range(3):
                p = ((iKRt[k, 0] * x + iKRt[k, 1] * y) + iKRt[k, 2] * dd) + iKRt[k, 3] * F(1)      # _iKRt * (j d, i d, d, 1)
                q = t["points"][it, k]
                num = q * pt + p * peso
                exact = num / somma
                fma = ((q.astype(np.float64) * pt.astype(np.float64) + (p * peso).astype(np.float64)).astype(F)) / somma
                rcp = num * (F(1) / somma)
                diff["fma"] += int((raw_bits(fma) != raw_bits(exact)).sum()); diff["rcp"] += int((raw_bits(rcp) != raw_bits(exact)).sum())
                t["points"][it, k] = dict(fma=fma, rcp=rcp).get(variant, exact)
            t["weights"][it] = somma
            # the appends, in raster order of their pixels
            rr, cc = np.nonzero(app)
            by_column = np.lexsort((rr, cc))
            diff["column_order"] += int((by_column != np.arange(len(rr))).sum())
            if variant == "column_order":
                rr, cc = rr[by_column], cc[by_column]
            _append(t, a, g, idx_c[rr, cc], F(1) / d[rr, cc])
            appended.append(int(app.sum())); fused.append(int(fuse.sum()))
    return t, np.array(appended, np.int32), np.array(fused, np.int32), counts, diff


def merge_list_literal(total, sources, transforms, proj, gauss=False):
    """merger2.cpp:106-183 as written, one pixel at a time -> (total, appended[n], fused[n])"""
    t = copy_total(total)
    K, offset, mn, mx, rows, cols = proj
    mn, mx = F(mn), F(mx)
    appended, fused = [], []
    with np.errstate(all="ignore"):
        for src, T in zip(sources, transforms):
            a, g = pushed_back(src, T, gauss)
            idx_c, dep_c, idx_t, dep_t, iKRt = _projections(t, src.arrays()["points"], T, proj)
            P, W = t["points"], t["weights"]
            push, pesi, nf = [], [], 0
            for i in range(rows):
                for j in range(cols):
                    d = dep_c[i, j]
                    if not (float(d) > 0.2 and float(d) < 100):
                        continue
                    peso = F(F(1) / d)
                    if idx_t[i, j] < 0:
                        push.append(idx_c[i, j]); pesi.append(peso)
                        continue
                    delta = F(d - dep_t[i, j])
                    if float(np.abs(delta)) < .15:
                        if d < mn or d > mx:                                       # unProject returns false
                            continue
                        x, y = F(F(j) * d), F(F(i) * d)
                        index = idx_t[i, j]
                        peso_tot = W[index]
                        somma = F(peso_tot + peso)
                        for k in range(3):
                            p = F(F(F(F(iKRt[k, 0] * x) + F(iKRt[k, 1] * y)) + F(iKRt[k, 2] * d)) + F(iKRt[k, 3] * F(1)))
                            P[index, k] = F(F(F(P[index, k] * peso_tot) + F(p * peso)) / somma)
                        W[index] = somma
                        nf += 1
                    elif float(delta) < -.3:
                        push.append(idx_c[i, j]); pesi.append(peso)
            _append(t, a, g, np.array(push, np.int64), np.array(pesi, F))
            appended.append(len(push)); fused.append(nf)
    return t, np.array(appended, np.int32), np.array(fused, np.int32)


def node_transform(bigT, nodeT):
    """T = big.transform()^-1 * node.transform() in double, cast to float (pwn_merger.cpp:36, :49-51)"""
    return (np.linalg.inv(np.asarray(bigT, np.float64)) @ np.asarray(nodeT, np.float64)).astype(F)


# ------------------------------------------------------------------------------------------------------------ natural input
OFFSET = np.array([[0, 0, 1, 0.1], [-1, 0, 0, 0.02], [0, -1, 0, 0.3], [0, 0, 0, 1]], F)      # a typical sensor mounting (tests/test_scene.py)


def converter_conf(rows):
    from oracle import oracle as O
    return dict(O.QVGA4_CONF_CONVERTER if rows <= 120 else O.VGA_CONF_CONVERTER)


@functools.lru_cache(maxsize=None)
def natural_case(rows=60, cols=80, K=K_SMALL, seed=3, n=9, with_offset=False):
    """n key frames of the seeded room along synth.trajectory(seed, n, t_step=0.08, r_step_deg=4.0), converted by the oracle with Stats and
    Gaussians under the sensor offset; the robot pose of frame k is camera pose * offset^-1 and T_k = pose_0^-1 * pose_k (mergeNodeList).
    The merger's projector is the converter's (same range).  -> dict(frames, robot poses, clouds, transforms, proj, conf, offset)"""
    from g2o_frontend_amd import synth
    from oracle import oracle as O
    cam = synth.trajectory(seed, n, t_step=0.08, r_step_deg=4.0)
    frames = [O.convert_16u_to_32f(synth.render_depth_mm(seed, cam[k], rows, cols, K, hole_stream=k)) for k in range(n)]
    offset = OFFSET if with_offset else EYE
    conf = converter_conf(rows)
    cp = O.converter_params(K, sensor_offset=offset if with_offset else None, **conf)
    O.set_gaussians(True)
    try:
        clouds = [O.convert(cp, f)[0] for f in frames]
    finally:
        O.set_gaussians(False)
    poses = [np.asarray(c, np.float64) @ np.linalg.inv(offset.astype(np.float64)) for c in cam]
    transforms = [node_transform(poses[0], p) for p in poses]
    transforms[0] = EYE.copy()                       # the big node itself: inverse * itself, the identity up to rounding -- made exact here
    proj = (K, offset, conf["min_distance"], conf["max_distance"], rows, cols)
    return dict(rows=rows, cols=cols, K=K, frames=frames, poses=poses, clouds=clouds, transforms=transforms, proj=proj, conf=conf, offset=offset)


def stripped(cloud):
    """the same points without Stats and Gaussians: what an uploaded cloud carries"""
    from oracle import oracle as O
    a = cloud.arrays()
    return O.Cloud.from_arrays(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])


# ----------------------------------------------------------------------------------------------------------- injected input
REPEAT = 8          # pixels per label
WIDE, NARROW = (0.1, 120.0), (0.5, 4.5)      # projector ranges: around the loop's (0.2, 100) / inside it, so that the range itself decides


def _ulps(x, k):
    v = F(x)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf), dtype=F)
    return v


def camera(rows, cols):
    return (100.0, 100.0, (cols - 1) / 2.0, (rows - 1) / 2.0)


def injected_labels(rng_name):
    """label -> (z of the incoming point, z of the total's point or None, expected action).  Identity cameras: d = z, depthImage_tot = z_tot."""
    mn, mx = WIDE if rng_name == "wide" else NARROW
    lab = {}
    base = F(1.5)
    ks = (-2, -1, 0, 1, 2)
    if rng_name == "wide":
        for name, x in (("lo", 0.2), ("hi", 100.0)):            # the loop's depth window, float against double
            for k in ks:
                z = _ulps(x, k)
                inside = float(z) > 0.2 and float(z) < 100
                lab["%s%+d/fresh" % (name, k)] = (z, None, "append_new" if inside else "drop_depth")
                lab["%s%+d/filled" % (name, k)] = (z, z, "fuse" if inside else "drop_depth")
    else:
        for name, x in (("min", mn), ("max", mx)):              # the projector's range: outside it the point does not reach the image at all
            for k in ks:
                z = _ulps(x, k)
                inside = not (z < F(mn) or z > F(mx))
                lab["%s%+d/fresh" % (name, k)] = (z, None, "append_new" if inside else "drop_depth")
                lab["%s%+d/filled" % (name, k)] = (z, base if name == "min" else F(4.4), ("append_occluder" if name == "min" else "fuse") if inside else "drop_depth")
    for sign in (1, -1):                                          # |d - depth_tot| around 0.15 on both sides of the total
        for k in ks:
            z = _ulps(F(base + F(sign * .15)), sign * k)
            within = float(np.abs(F(z - base))) < .15
            lab["near%s%+d" % ("+" if sign > 0 else "-", k)] = (z, base, "fuse" if within else "drop_between")
    for k in ks:                                                  # d - depth_tot around -0.3
        z = _ulps(F(base + F(-.3)), k)
        lab["occluder%+d" % k] = (z, base, "append_occluder" if float(F(z - base)) < -.3 else "drop_between")
    lab["behind"] = (F(2.25), base, "drop_between")              # 0.75 behind the total
    lab["plain/fresh"] = (F(1.75), None, "append_new")
    lab["plain/filled"] = (F(1.75), F(1.8), "fuse")
    return lab


def _cloud_arrays(rng, pix, z, K, rows, cols, jitter=0.3, nonfinite=None):
    """points on the rays through the pixels `pix` at depths z (identity camera: z is the depth in every bit), up to `jitter` pixel off the
    centre; unit normals, curvatures, exactly symmetric Omega_p, Omega_n = 100 I"""
    n = len(pix)
    fx, fy, cx, cy = K
    r, c = np.asarray(pix) // cols, np.asarray(pix) % cols
    z = np.asarray(z, F)
    u = c + rng.uniform(-jitter, jitter, n); v = r + rng.uniform(-jitter, jitter, n)
    pts = np.zeros((n, 4), F)
    pts[:, 0] = ((u - cx) / fx * z.astype(np.float64)).astype(F); pts[:, 1] = ((v - cy) / fy * z.astype(np.float64)).astype(F); pts[:, 2] = z; pts[:, 3] = 1
    nrm = np.zeros((n, 4), F)
    v3 = rng.standard_normal((n, 3)) * 0.3 + np.array([0, 0, -1.0]); nrm[:, :3] = (v3 / np.linalg.norm(v3, axis=1, keepdims=True)).astype(F)
    curv = rng.uniform(0, 0.05, n).astype(F)
    A = rng.standard_normal((n, 3, 3)).astype(F)
    S = (A @ A.transpose(0, 2, 1) + np.eye(3, dtype=F)).astype(F)
    S = np.triu(S) + np.triu(S, 1).transpose(0, 2, 1)                        # exactly symmetric
    if nonfinite is not None:
        for m, i in enumerate(np.nonzero(nonfinite)[0]):
            kind = m % 3
            if kind == 0: S[i, 0, 0] = np.inf
            elif kind == 1: S[i, 0, 1] = S[i, 1, 0] = np.nan
            else: S[i, 2, 2] = -np.inf; S[i, 1, 2] = S[i, 2, 1] = np.inf
    op = np.zeros((n, 16), F); on = np.zeros((n, 16), F)
    for a in range(3):
        for b in range(3):
            op[:, a + 4 * b] = S[:, a, b]
        on[:, a + 4 * a] = 100
    return dict(points=pts, normals=nrm, curvature=curv, omega_p=op, omega_n=on)


def _concat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _shuffled(rng, a):
    perm = rng.permutation(len(a["points"]))
    return {k: v[perm] for k, v in a.items()}


def injected_case(rows, cols, n, ranges="wide", moved=False, seed=0):
    """A pre-filled total and a list of n incoming clouds of rows x cols.  Cloud 0 (A) carries the labels, REPEAT pixels each where the image
    holds them (cyclically otherwise); some of its pixels hold two and three points (the nearest decides, ties go to the lower index), some
    appended points have a non-finite Omega_p; one point of the total carries a weight summed over 8 contributors.  The list is A, A again,
    an empty cloud, a cloud wholly behind the camera, then seeded clouds around what is there.  moved: the later clouds come under small
    non-identity transforms and everything under a non-identity sensor offset (the labels then only populate the branches).
    -> dict(total (arrays), weights, sources (arrays per cloud), transforms, proj, label_pixels, expect)"""
    rng = np.random.default_rng(seed + 1000 * rows + cols + (7 if ranges == "narrow" else 0))
    N = rows * cols
    K = camera(rows, cols)
    mn, mx = WIDE if ranges == "wide" else NARROW
    lab = injected_labels(ranges)
    names = sorted(lab)
    pix = np.arange(N)
    name_of = [names[(i // REPEAT) % len(names)] if N >= REPEAT * len(names) else names[i % len(names)] for i in range(N)]
    label_pixels = {k: [] for k in names}
    for i, nm in enumerate(name_of):
        label_pixels[nm].append(i)
    zc = np.array([lab[nm][0] for nm in name_of], F)
    has_t = np.array([lab[nm][1] is not None for nm in name_of])
    zt = np.array([lab[nm][1] if lab[nm][1] is not None else 0 for nm in name_of], F)
    fresh = np.array([nm.endswith("fresh") for nm in name_of])
    # cloud A: the labelled point of every pixel, plus farther points on every 5th / 11th pixel (two / three points in a pixel) and an equal-depth
    # twin on every 13th (the tie: the lower index wins)
    A = [_cloud_arrays(rng, pix, zc, K, rows, cols, nonfinite=fresh & (pix % 3 == 0))]
    for step, dz in ((5, 0.25), (11, 0.5)):
        sub = pix[(pix % step == 0) & (zc < 50) & (zc >= F(mn)) & (zc <= F(mx))]      # behind a point that reaches the image
        A.append(_cloud_arrays(rng, sub, zc[sub] + F(dz), K, rows, cols))
    sub = pix[pix % 13 == 0]
    A.append(_cloud_arrays(rng, sub, zc[sub], K, rows, cols))
    A = _shuffled(rng, _concat(A))
    # the total: its labelled points, a second (farther) point on every 7th filled pixel
    tp = pix[has_t]
    T0 = [_cloud_arrays(rng, tp, zt[tp], K, rows, cols)]
    sub = tp[tp % 7 == 0]
    T0.append(_cloud_arrays(rng, sub, zt[sub] + F(0.4), K, rows, cols))
    T0 = _shuffled(rng, _concat(T0))
    w0 = (F(1) / T0["points"][:, 2]).astype(F)
    if len(w0):                                                   # a weight already summed over 8 contributors
        heavy = int(np.argmin(np.abs(T0["points"][:, 2] - F(1.8)))) if ranges == "wide" else 0
        acc = F(0)
        for _ in range(8):
            acc = F(acc + F(F(1) / T0["points"][heavy, 2]))
        w0[heavy] = acc
    sources = [A, A]
    sources.append({k: v[:0] for k, v in A.items()})             # empty
    behind = {k: v.copy() for k, v in A.items()}; behind["points"][:, :3] *= F(-1)
    sources.append(behind)
    base = rng.uniform(0.8, 3.5, N).astype(F)
    while len(sources) < n:
        jit = rng.choice(np.array([0, 0.01, -0.02, 0.14, -0.14, 0.16, -0.16, -0.29, -0.31, -0.5, 0.9], F), N)
        keep = rng.random(N) > 0.15
        sources.append(_shuffled(rng, _cloud_arrays(rng, pix[keep], (base + jit)[keep], K, rows, cols)))
    sources = sources[:n]
    transforms = [EYE.copy() for _ in range(n)]
    offset = EYE.copy()
    if moved:
        from g2o_frontend_amd import synth
        offset = OFFSET.copy()
        for i in range(1, n):
            transforms[i] = synth.v2t(np.array([0.01 * i, -0.015, 0.02, 0.004 * i, -0.003, 0.005])).astype(F)
        off64 = offset.astype(np.float64)

        def to_robot(a):                                          # camera frame -> robot frame (the cloud as the converter would store it)
            a = {k: v.copy() for k, v in a.items()}
            a["points"][:, :3] = (a["points"][:, :3].astype(np.float64) @ off64[:3, :3].T + off64[:3, 3]).astype(F)
            return a
        sources = [to_robot(s) for s in sources]; T0 = to_robot(T0)
    expect = {nm: lab[nm][2] for nm in names}
    return dict(rows=rows, cols=cols, total=T0, weights=w0, sources=sources, transforms=transforms, proj=(K, offset, mn, mx, rows, cols),
                label_pixels=label_pixels, expect=expect, moved=moved)


SHAPES = [(1, 1), (1, 65), (9, 65), (17, 129), (60, 80), (120, 160)]      # 17 x 129 = 2 193 pixels: two 1024-blocks of the scan and a partial third


def injected_variants(rows, cols):
    """(n, ranges, moved) of the injected lists at a shape: n = 1, 2, 3 and 9, both projector ranges, identity and non-identity transforms / offset"""
    v = [(1, "wide", False), (2, "narrow", False), (3, "wide", True), (9, "wide", False)]
    if (rows, cols) == (17, 129):
        v += [(3, "narrow", False), (3, "wide", False), (9, "narrow", True)]
    return v


def oracle_clouds(case):
    """the injected clouds as oracle clouds (identical arrays share one cloud, so that the same cloud comes twice in the list)"""
    from oracle import oracle as O
    made = {}
    out = []
    for s in case["sources"]:
        if id(s) not in made:
            made[id(s)] = O.Cloud.from_arrays(s["points"], s["normals"], s["curvature"], s["omega_p"], s["omega_n"])
        out.append(made[id(s)])
    return out
