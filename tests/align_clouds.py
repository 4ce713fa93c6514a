"""Injected clouds for the aligner's fused pass (k_corr_linearize / k_corr_linearize_lat), its list twin (k_linearize_list) and the solve step
(k_solve_update): pairs of clouds built pixel by pixel so that the branches and edges converter-made clouds hardly reach are dense.  A helper
module of the tests, imported by test_align_clouds_cpu.py and test_gpu_align_clouds.py; the clouds reach the GPU through
pwn_hip_cloud_upload (full Omega_n planes) and the oracle through Cloud.from_arrays.

A case holds a reference and a current cloud as arrays, an image size, the camera, a guess T, its aligner parameters and a family / sub-kind
label per pixel.  A point for pixel (r, c) at depth d lies on the ray through the pixel's centre (the reference point up to 0.2 pixel off it).
The LAYOUT is written in the current frame; the stored reference cloud is T * layout (Aligner::align projects the reference through T^-1 and
tests T^-1 * p against the current point).  Under the identity guess iso_point / iso_normal return their input bits, so thresholds are hit
exactly: a pixel gets 48 variants of its free parameter, the tested quantity is evaluated in fp32 in the reference's operation order and the
variant at the wanted ulp distance from the threshold is kept.  Under another guess the stored cloud is the layout carried through T in
float64 and rounded, and thresholds are met by log-spaced ladders (1e-7.5 .. 1e-3 either side).  Points are stored in a random permutation.

Families (FAMILIES): zero_normal, normal_angle, distance, ratio, chi2_edge, omega_range, cancel, index_edges, empty; their sub-kinds are the
`sub` labels.  Every Omega is positive semi-definite up to rounding, every point finite.  class_edge (the last family, in no mixed case) is for
clouds of the converter's form (tests/flat_clouds.py), whose Omega_n is a class matrix chosen by the current point's curvature against the
cloud's threshold cls_thr: current curvatures at cls_thr, reference curvatures on its other side.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
TILE = 2048                      # pixels per workgroup of the fused pass: kPixPerThread * kAlignBlock (pwn_kernels.h)
CHAIN = 8                        # kPixPerThread
PARAMS = dict(min_distance=0.5, max_distance=4.5, inlier_distance_threshold=1.0, inlier_normal_angular_threshold=0.95,
              flat_curvature_threshold=0.02, inlier_curvature_ratio_threshold=1.3, inlier_max_chi2=9000.0, robust_kernel=1,
              outer_iterations=1, inner_iterations=1)
FAMILIES = ("zero_normal", "normal_angle", "distance", "ratio", "chi2_edge", "omega_range", "cancel", "index_edges", "empty", "class_edge")
VARIANTS = 48
WANT = np.array([0, -1, 1, 0, -2, 2, 0, -3, 3, -4, 4])      # ulp distances from a threshold, dealt round-robin (equality three times as often)


def v2t64(v):
    """translation + vector part of a unit quaternion -> 4x4, float64"""
    x, y, z = v[3:6]; w = np.sqrt(max(0.0, 1.0 - x * x - y * y - z * z))
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + z * w), w * w - x * x + y * y - z * z, 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), w * w - x * x - y * y + z * z]])
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = v[:3]
    return T


def axis_angle(axis, degrees, t=(0.0, 0.0, 0.0)):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    th = np.deg2rad(degrees)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx); T[:3, 3] = t
    return T


GUESSES = {"identity": np.eye(4), "small": v2t64(np.array([0.03, -0.02, 0.05, 0.01, -0.015, 0.02])),
           "moderate": v2t64(np.array([-0.2, 0.1, 0.3, -0.05, 0.04, 0.03]))}
# rotations beyond 120 degrees: the trace <= 0 branches of mat2quat (largest diagonal entry 0, 1, 2 for x, y, z; 2 for the skew axis)
BIG_AXES = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1), "skew": (1, 2, 3)}
BIG_ANGLES = (125.0, 150.0, 179.0, 180.0)


def big_guesses():
    out = {}
    for i, (an, ax) in enumerate(BIG_AXES.items()):
        for j, deg in enumerate(BIG_ANGLES):
            out[f"{an}{deg:g}"] = axis_angle(ax, deg, (0.3 - 0.1 * i, -0.2 + 0.15 * j, 0.1 * (i - j)))
    return out


def camera(rows, cols):
    return (525.0, 525.0, (cols - 1) / 2.0, (rows - 1) / 2.0)


def ulps(a, t):
    """signed distance in float32 steps of the positive floats a from the positive float t"""
    return np.asarray(a, F32).view(np.int32).astype(np.int64) - int(np.array(t, F32).view(np.int32))


def dot3(a, b):
    """(a0 b0 + a1 b1) + a2 b2 in fp32: dot4seq with an exact-zero fourth product"""
    a = np.asarray(a, F32); b = np.asarray(b, F32)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _frames(n1):
    """orthonormal frames [n, 3, 3] whose first column is n1 (float64)"""
    h = np.where(np.abs(n1[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    u = _unit(np.cross(n1, h)); w = np.cross(n1, u)
    return np.stack([n1, u, w], 2)


def omega_converter(U, dg):
    """U diag(dg) U^t as informationmatrixcalculator.cpp:26-30 evaluates it in fp32: nine separately rounded entries, symmetric up to rounding"""
    U = U.astype(F32); dg = np.asarray(dg, F32)
    om = np.zeros((len(U), 3, 3), F32)
    for i in range(3):
        for j in range(3):
            om[:, i, j] = ((U[:, i, 0] * dg[:, 0]) * U[:, j, 0] + (U[:, i, 1] * dg[:, 1]) * U[:, j, 1]) + (U[:, i, 2] * dg[:, 2]) * U[:, j, 2]
    return om


def _choose(k, want):
    """per row of k [n, m]: the column whose value equals want, else the one nearest to it"""
    d = np.abs(k - want[:, None])
    return np.argmin(d, axis=1)


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def pixels(self):
        return self.rows * self.cols

    @property
    def tiles(self):
        return (self.pixels + TILE - 1) // TILE

    def candidates(self, fam=None):
        m = (self.ref_index.reshape(-1) >= 0) & (self.cur_index.reshape(-1) >= 0)
        return m if fam is None else m & (self.family == fam)


class _Builder:
    def __init__(self, rng, rows, cols, K, exact, params, cls_thr=0.02):
        self.rng, self.rows, self.cols, self.K, self.exact, self.params, self.cls_thr = rng, rows, cols, K, exact, params, cls_thr
        self.N = rows * cols
        self.free = np.ones(self.N, bool)
        self.family = np.full(self.N, "", object); self.sub = np.full(self.N, "", object); self.expect = np.full(self.N, -1, np.int8)
        self.recs = {"ref": [], "cur": []}

    # ---- pixels
    def take(self, n, allowed, pair_delta=0):
        ok = self.free & allowed
        if pair_delta:
            c = np.arange(self.N) % self.cols
            sh = np.zeros(self.N, bool); sh[:-pair_delta] = ok[pair_delta:]
            ok = ok & sh & (c + pair_delta < self.cols)
        idx = np.nonzero(ok)[0]
        self.rng.shuffle(idx)
        out = []
        for p in idx:                                   # pairs must not overlap
            if len(out) >= n:
                break
            if self.free[p] and (not pair_delta or self.free[p + pair_delta]):
                out.append(p); self.free[p] = False
                if pair_delta:
                    self.free[p + pair_delta] = False
        return np.array(sorted(out), np.int64)

    def rays(self, pix, jitter=None):
        fx, fy, cx, cy = self.K
        r, c = pix // self.cols, pix % self.cols
        x = (c - cx) / fx; y = (r - cy) / fy
        if jitter is not None:
            x = x + jitter[..., 0] / fx; y = y + jitter[..., 1] / fy
        return np.stack([x, y, np.ones_like(x)], -1)

    def base(self, pix, far=False):
        rng, n = self.rng, len(pix)
        d = rng.uniform(4.2, 4.45, n) if far else rng.uniform(1.0, 3.5, n)
        dirc = self.rays(pix)
        cpos = (dirc * d[:, None]).astype(F32).astype(np.float64)
        rdir = self.rays(pix, rng.uniform(-0.2, 0.2, (n, 2)))
        rpos = (rdir * (d + rng.uniform(-0.02, 0.02, n))[:, None]).astype(F32).astype(np.float64)
        cn = _unit(-_unit(dirc) + 0.3 * rng.standard_normal((n, 3))).astype(F32).astype(np.float64)
        rn = _unit(cn + 0.03 * rng.standard_normal((n, 3))).astype(F32).astype(np.float64)
        Op = omega_converter(_frames(_unit(cn)), np.tile(np.array([[1000.0, 1.0, 1.0]]), (n, 1)))
        On = np.tile((np.eye(3) * 100.0).astype(F32), (n, 1, 1))
        return dict(pix=pix, cpos=cpos, rpos=rpos, cn=cn, rn=rn, ccurv=rng.uniform(0, 0.015, n).astype(F32), rcurv=rng.uniform(0, 0.015, n).astype(F32),
                    Op=Op, On=On, sub=np.full(n, "", object), expect=np.full(n, -1, np.int8))

    def put(self, fam, b):
        n = len(b["pix"])
        self.family[b["pix"]] = fam; self.sub[b["pix"]] = b["sub"]; self.expect[b["pix"]] = b["expect"]
        rOp = omega_converter(_frames(_unit(np.where(np.abs(b["rn"]).sum(1, keepdims=True) > 1e-20, b["rn"], [[0, 0, 1.0]]))), np.tile(np.array([[1000.0, 1.0, 1.0]]), (n, 1)))
        self.add("cur", b["pix"], b["cpos"], b["cn"], b["ccurv"], b["Op"], b["On"])
        self.add("ref", b["pix"], b["rpos"], b["rn"], b["rcurv"], rOp, b["On"])

    def add(self, side, pix, pos, nrm, curv, Op, On, visible=None):
        n = len(pix)
        self.recs[side].append(dict(pix=np.asarray(pix, np.int64), pos=np.asarray(pos, np.float64), nrm=np.asarray(nrm, np.float64), curv=np.asarray(curv, F32),
                                    Op=np.asarray(Op, F32), On=np.asarray(On, F32), visible=np.ones(n, bool) if visible is None else np.asarray(visible, bool)))

    # ---- families
    def zero_normal(self, pix):
        b = self.base(pix); n = len(pix)
        # denorm: components near 1e-21, squares (1e-42) denormal, the sum nonzero: must pass.  (1e-23 itself squares to 1e-46, below the smallest
        # denormal 1.4e-45, and would underflow like 1e-30 does.)  under: components near 1e-30, squares underflow to 0: rejected.
        kinds = ["zero_ref", "zero_cur", "zero_both", "denorm_ref", "denorm_cur", "denorm_both", "under_ref", "under_cur", "under_both"]
        passes = self.params["inlier_normal_angular_threshold"] <= 0.0
        b["rn"] = b["cn"].copy()                                    # same direction: a tiny normal keeps cN . rn > 0
        for i in range(n):
            k = kinds[i % len(kinds)]; b["sub"][i] = k
            s = 0.0 if k.startswith("zero") else (1e-21 if k.startswith("denorm") else 1e-30) * self.rng.uniform(0.6, 1.6)
            if k.endswith("ref") or k.endswith("both"):
                b["rn"][i] = b["rn"][i] * s
            if k.endswith("cur") or k.endswith("both"):
                b["cn"][i] = b["cn"][i] * s
            b["expect"][i] = 1 if (k.startswith("denorm") and passes) else 0
        return b

    def _ladder(self, n):
        return self.rng.choice([-1.0, 1.0], n) * 10.0 ** self.rng.uniform(-7.5, -3.0, n)

    def normal_angle(self, pix):
        b = self.base(pix); n = len(pix); rng = self.rng
        thr = float(F32(self.params["inlier_normal_angular_threshold"]))
        cn = b["cn"]; a = _frames(_unit(cn))[:, :, 1]
        if self.exact:
            th = np.arccos(thr) + rng.uniform(-1e-6, 1e-6, (n, VARIANTS))
            rn = (np.cos(th)[..., None] * cn[:, None] + np.sin(th)[..., None] * a[:, None]).astype(F32)
            j = _choose(ulps(dot3(cn[:, None].astype(F32), rn), thr), WANT[np.arange(n) % len(WANT)])
            b["rn"] = rn[np.arange(n), j].astype(np.float64); b["sub"][:] = "exact"
        else:
            th = np.arccos(np.clip(thr + self._ladder(n), -1, 1))
            b["rn"] = np.cos(th)[:, None] * cn + np.sin(th)[:, None] * a; b["sub"][:] = "ladder"
        return b

    def distance(self, pix):
        b = self.base(pix); n = len(pix); rng = self.rng
        L0 = float(F32(self.params["inlier_distance_threshold"]))
        near = rng.random(n) < 0.5                               # the reference point beyond the current one, or in front of it
        d = np.where(near, rng.uniform(0.8, 2.0, n), rng.uniform(2.8, 4.0, n))
        q = (self.rays(pix) * d[:, None]).astype(F32).astype(np.float64)
        m = VARIANTS if self.exact else 1
        L = L0 + (rng.uniform(-1.5e-6, 1.5e-6, (n, m)) if self.exact else self._ladder(n)[:, None])
        rdir = self.rays(pix, rng.uniform(-0.2, 0.2, (n, 2)))        # along the ray, and up to 0.2 pixel across it
        A = (rdir * rdir).sum(1)[:, None]; B = (rdir * q).sum(1)[:, None]; Cq = (q * q).sum(1)[:, None] - L * L
        root = np.sqrt(B * B - A * Cq)
        dr = np.where(near[:, None], (B + root) / A, (B - root) / A)
        rpos = (rdir[:, None] * dr[..., None]).astype(F32)
        if self.exact:
            df = q[:, None].astype(F32) - rpos
            j = _choose(ulps(dot3(df, df), F32(L0) * F32(L0)), WANT[np.arange(n) % len(WANT)])
        else:
            j = np.zeros(n, np.int64)
        b["cpos"] = q; b["rpos"] = rpos[np.arange(n), j].astype(np.float64); b["rn"] = b["cn"].copy()
        b["sub"][:] = "exact" if self.exact else "ladder"
        return b

    def ratio(self, pix):
        b = self.base(pix); n = len(pix); rng = self.rng
        flat = F32(self.params["flat_curvature_threshold"]); mx = F32(self.params["inlier_curvature_ratio_threshold"]); mn = F32(1.0) / mx
        edge = [np.nextafter(flat, F32(0)), flat, np.nextafter(flat, F32(1)), F32(0.0)]
        kinds = ["bound", "band", "bound", "band", "flat", "band", "zero", "clamped"]
        for i in range(n):
            k = kinds[i % len(kinds)]; b["sub"][i] = k
            t = float(mn if (i // len(kinds)) % 2 else mx)
            cc = F32(rng.uniform(0.03, 0.3))
            if k == "bound":                                        # the double-evaluated, float-rounded ratio at the bound, 0..3 ulps either side
                rc0 = F32(t * (float(cc) + 1e-5) - 1e-5)
                var = np.array([rc0], F32)
                lo, hi = rc0, rc0
                for _ in range(8):
                    lo = np.nextafter(lo, F32(0)); hi = np.nextafter(hi, F32(1)); var = np.concatenate([var, [lo, hi]])
                r = ((var.astype(np.float64) + 1e-5) / (float(cc) + 1e-5)).astype(F32)
                want = [0, -1, 1, -2, 2, -3, 3][(i // len(kinds)) % 7]
                rc = var[np.argmin(np.abs(ulps(r, t) - want))]
            elif k == "band":                                       # across the +-1e-5 band of the fp32 estimate, both sides of both bounds
                u = rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-7.0, -4.3)
                rc = F32(t * (1 + u) * (float(cc) + 1e-5) - 1e-5)
            elif k == "flat":                                       # below, at and above flatThr on each side
                rc = edge[(i // len(kinds)) % 3]; cc = edge[(i // (3 * len(kinds))) % 3]
            elif k == "zero":
                rc = F32(0.0) if (i // len(kinds)) % 3 != 1 else F32(rng.uniform(0, 0.025)); cc = F32(0.0) if (i // len(kinds)) % 3 != 2 else F32(rng.uniform(0, 0.025))
            else:
                rc = F32(rng.uniform(0, 0.02)); cc = F32(rng.uniform(0, 0.02))
            b["rcurv"][i] = rc; b["ccurv"][i] = cc
        return b

    def _local_error(self, b, Op):
        """localError (linearizer.cpp:52-62) in fp32, identity guess: rp / rn are the stored bits"""
        pe = b["rpos"].astype(F32) - b["cpos"].astype(F32); ne = b["rn"].astype(F32) - b["cn"].astype(F32)
        def mv(o, v): return np.stack([dot3(o[..., k, :], v) for k in range(3)], -1)
        if Op.ndim == 4:
            pe = pe[:, None]; ne = ne[:, None]; On = b["On"][:, None]
        else:
            On = b["On"]
        return dot3(pe, mv(Op, pe)) + dot3(ne, mv(On, ne))

    def chi2_edge(self, pix):
        b = self.base(pix); n = len(pix); rng = self.rng
        mc = float(F32(self.params["inlier_max_chi2"]))
        d = (b["cpos"] ** 2).sum(1) ** 0.5
        b["rpos"] = (b["cpos"] * (1 + rng.choice([-1, 1], n) * rng.uniform(0.05, 0.3, n) / d)[:, None]).astype(F32).astype(np.float64)
        M = np.einsum("nij,nj,nkj->nik", _frames(_unit(b["cn"])), np.stack([np.ones(n), rng.uniform(0.2, 0.5, n), rng.uniform(0.05, 0.2, n)], 1), _frames(_unit(b["cn"])))
        M = (M + M.transpose(0, 2, 1)) / 2                                             # exactly symmetric: the same matrix in both storages
        pe = b["rpos"] - b["cpos"]; ne = b["rn"] - b["cn"]
        a = np.einsum("ni,nij,nj->n", pe, M, pe); c = np.einsum("ni,nij,nj->n", ne, b["On"].astype(np.float64), ne)
        lam0 = (mc - c) / a
        above = (np.arange(n) % 4) == 3                                                # every fourth: 1e3 .. 1e8 times above (tiny kscale)
        if self.exact:
            lam = lam0[:, None] * (1 + rng.uniform(-4e-7, 4e-7, (n, VARIANTS)))
            Ov = (lam[..., None, None] * M[:, None]).astype(F32)
            j = _choose(ulps(self._local_error(b, Ov), mc), WANT[np.arange(n) % len(WANT)])
            Op = Ov[np.arange(n), j]
        else:
            Op = ((lam0 * (1 + self._ladder(n)))[:, None, None] * M).astype(F32)
        Op[above] = ((lam0[above] * 10.0 ** rng.uniform(3, 8, int(above.sum())))[:, None, None] * M[above]).astype(F32)
        b["Op"] = Op; b["sub"][:] = "exact" if self.exact else "ladder"; b["sub"][above] = "above"
        return b

    def omega_range(self, pix):
        b = self.base(pix); n = len(pix); rng = self.rng
        U = _frames(_unit(b["cn"] + 0.2 * rng.standard_normal((n, 3))))
        kinds = ["flat", "inv_lambda", "zero", "flat", "inv_lambda"]
        dg = np.tile(np.array([[1000.0, 1.0, 1.0]]), (n, 1))
        for i in range(n):
            k = kinds[i % len(kinds)]; b["sub"][i] = k
            if k == "inv_lambda":                                                       # 1 / lambda of the non-flat branch, up to 1e10
                dg[i] = np.sort(10.0 ** rng.uniform(0, [10.0, 6.0, 3.0]))[::-1]
            elif k == "zero":
                dg[i] = 0.0
        b["Op"] = omega_converter(U, dg)
        A = rng.standard_normal((n, 3, 3)) * (10.0 ** rng.uniform(-1, 1.5, n))[:, None, None]      # a different full Omega_n per point
        b["On"] = np.einsum("nij,nkj->nik", A, A).astype(F32)
        return b

    def cancel(self, pix, delta):
        """pairs (p, p + delta): Omega' = D Omega D (1 + eps), pe' = -D pe with D = diag(1, 1, -1): b_t[0:2], Htt[0:2, 2] and the Htr entries built
        from Omega[0:2, 2] cancel to eps = 1e-6 .. 1e-4 of the sum of their magnitudes; points at the far end of the depth range"""
        rng, n = self.rng, len(pix)
        both = np.concatenate([pix, pix + delta])
        b = self.base(both, far=True)
        d = rng.uniform(4.2, 4.45, n); d = np.concatenate([d, d])
        b["cpos"] = (self.rays(both) * d[:, None]).astype(F32).astype(np.float64)
        D = np.array([1.0, 1.0, -1.0])
        e = _unit(self.rays(pix)) * rng.uniform(5e-4, 1e-3, n)[:, None] * rng.choice([-1, 1], n)[:, None]
        pe = np.concatenate([e, -e * D])
        b["rpos"] = (b["cpos"] + pe).astype(F32).astype(np.float64)
        ang = rng.uniform(0.3, 1.2, n); nn = np.stack([np.sin(ang), np.zeros(n), np.cos(ang)], 1)
        lam = 10.0 ** rng.uniform(2, 4, n)
        Om = lam[:, None, None] * nn[:, :, None] * nn[:, None, :] + np.eye(3)
        eps = rng.choice([-1, 1], n) * 10.0 ** rng.uniform(-6, -4, n)
        b["Op"] = np.concatenate([Om, Om * D[:, None] * D[None, :] * (1 + eps)[:, None, None]]).astype(F32)
        b["rn"] = b["cn"].copy(); b["On"] = np.tile(np.eye(3, dtype=F32), (2 * n, 1, 1))
        b["sub"][:] = f"pair+{delta}"
        return b

    def index_edges(self, pix, specials):
        """specials: pixels that must hold a plain candidate (pixel 0, pixel N - 1, whole thread columns, a tile's last pixel)"""
        rng = self.rng
        kinds = ["ref_only", "cur_only", "depth_below", "depth_above", "depth_at", "multi2", "multi3", "tie2", "tie3", "plain"]
        b = self.base(np.concatenate([pix, specials[0]]).astype(np.int64))
        n, m = len(pix), len(b["pix"])
        for i in range(m):
            b["sub"][i] = kinds[i % len(kinds)] if i < n else specials[1][i - n]
        sub = b["sub"]
        b["rn"] = _unit(b["cn"] + 0.01 * rng.standard_normal((m, 3)))
        self.family[b["pix"]] = "index_edges"; self.sub[b["pix"]] = sub
        lo, hi = F32(self.params["min_distance"]), F32(self.params["max_distance"])
        side_is_ref = rng.random(m) < 0.5
        for side in ("cur", "ref"):
            pos = b["cpos"].copy() if side == "cur" else b["rpos"].copy()
            nrm = b["cn"] if side == "cur" else b["rn"]
            mine = side_is_ref == (side == "ref")
            keep = ~np.isin(sub, ["ref_only" if side == "cur" else "cur_only"])
            visible = np.ones(m, bool)
            dirc = self.rays(b["pix"])
            for kind, z in (("depth_below", np.nextafter(lo, F32(0))), ("depth_above", np.nextafter(hi, F32(10))), ("depth_at", None)):
                sel = (sub == kind) & mine
                zz = np.where(rng.random(m) < 0.5, lo, hi).astype(np.float64) if z is None else np.full(m, float(z))
                if not self.exact and side == "ref":                 # the reference's depth is computed from T * layout: a margin instead of an ulp
                    zz = zz * (1 + {"depth_below": -1e-4, "depth_above": 1e-4}.get(kind, 0.0)) if kind != "depth_at" else np.where(zz == float(lo), zz * (1 + 1e-4), zz * (1 - 1e-4))
                pos[sel] = (dirc[sel] * zz[sel, None]).astype(F32)
                if kind != "depth_at":
                    visible[sel] = False
            self.add(side, b["pix"][keep], pos[keep], nrm[keep], (b["ccurv"] if side == "cur" else b["rcurv"])[keep], b["Op"][keep], b["On"][keep], visible[keep])
            # further points of the same cloud in the pixel: behind the winner (multi) or at its very position (tie: the lowest index wins);
            # they carry the opposite normal, so a wrong winner changes the correspondence list
            for kind, extra, step in (("multi2", 1, 0.1), ("multi3", 2, 0.1), ("tie2", 1, 0.0), ("tie3", 2, 0.0)):
                sel = np.nonzero((sub == kind) & mine)[0]
                for e in range(1, extra + 1):
                    p2 = pos[sel] * (1 + e * step / pos[sel][:, 2:3])
                    self.add(side, b["pix"][sel], p2.astype(F32), -nrm[sel] if step else nrm[sel] * (1 - 0.3 * e), rng.uniform(0, 0.015, len(sel)), b["Op"][sel] * F32(1 + e), b["On"][sel])

    def empty_none(self, pix):
        b = self.base(pix); n = len(pix)
        self.family[pix] = "empty"; self.sub[pix] = "none"; self.expect[pix] = 0
        h = n // 2
        self.add("cur", pix[:h], b["cpos"][:h], b["cn"][:h], b["ccurv"][:h], b["Op"][:h], b["On"][:h])
        self.add("ref", pix[h:], b["rpos"][h:], b["rn"][h:], b["rcurv"][h:], b["Op"][h:], b["On"][h:])

    def empty_rejected(self, pix):
        b = self.base(pix); b["rn"] = -b["cn"]; b["sub"][:] = "rejected"; b["expect"][:] = 0
        return b

    def class_edge(self, pix):
        """the current curvature at cls_thr, at equality and 1 .. 4 ulps either side (curvatures are stored bits: no variants needed, under any
        guess); in every second pixel the reference curvature on the OTHER side of cls_thr, by 1 ulp .. 5 % (sub "across"), else equal to the
        current one ("same").  Omega_n is the shipped table by the class rule, so the uploaded form of the case is the same cloud.  Every pair is
        a correspondence: the curvatures differ by 5 % at the most, the ratio stays near 1."""
        b = self.base(pix); n = len(pix); rng = self.rng
        thr = F32(self.cls_thr); tb = int(thr.view(np.int32))
        want = WANT[np.arange(n) % len(WANT)]
        cc = (tb + want).astype(np.int32).view(F32)
        below = cc < thr                                           # class 1 (flat); equality is class 2
        across = (np.arange(n) // len(WANT)) % 2 == 0
        steps = np.where(rng.random(n) < 0.4, rng.integers(1, 4, n), 0)                       # 1 .. 3 ulps, else a relative offset 1e-6 .. 5e-2
        rel = 10.0 ** rng.uniform(-6.0, np.log10(0.05), n)
        up = np.where(steps > 0, (tb + steps - 1).astype(np.int32).view(F32), (float(thr) * (1 + rel)).astype(F32))      # >= thr: class 2
        dn = np.where(steps > 0, (tb - steps).astype(np.int32).view(F32), (float(thr) * (1 - rel)).astype(F32))          # < thr: class 1
        rc = np.where(across, np.where(below, up, dn), cc).astype(F32)
        b["ccurv"] = cc.astype(F32); b["rcurv"] = rc
        b["On"] = np.where(below[:, None, None], (np.eye(3) * 100.0).astype(F32), np.eye(3, dtype=F32)).astype(F32)
        b["sub"][:] = np.where(across, "across", "same"); b["expect"][:] = 1
        return b


def _zbuffer(pix, key, visible, N):
    """the intended index image: nearest visible point per pixel, ties to the lowest index"""
    idx = np.nonzero(visible)[0]
    order = np.lexsort((idx, key[idx], pix[idx]))
    ps, is_ = pix[idx][order], idx[order]
    first = np.ones(len(ps), bool); first[1:] = ps[1:] != ps[:-1]
    out = np.full(N, -1, np.int32); out[ps[first]] = is_[first]
    return out


def make_case(name, rows, cols, guess, counts, seed, tiles=None, lone_tile=None, params=None, cls_thr=0.02):
    """counts: family -> number of pixels (cancel: pairs; empty: "none" or "rejected" pixels through the keys empty_none / empty_rejected).
    tiles: restrict the candidates to these 2048-pixel tiles; lone_tile: a tile whose only candidate is its last pixel."""
    rng = np.random.default_rng(seed)
    p = dict(PARAMS); p.update(params or {})
    G = np.asarray(GUESSES[guess] if isinstance(guess, str) else guess, np.float64)
    exact = bool(np.array_equal(G, np.eye(4)))
    K = camera(rows, cols)
    B = _Builder(rng, rows, cols, K, exact, p, cls_thr)
    N = rows * cols
    tile_of = np.arange(N) // TILE
    allowed = np.ones(N, bool) if tiles is None else np.isin(tile_of, list(tiles))
    if lone_tile is not None:
        allowed &= tile_of != lone_tile
    if "index_edges" in counts:
        sp, kinds = [], []
        def special(px, kind):
            if 0 <= px < N and B.free[px] and px not in sp:
                sp.append(px); kinds.append(kind); B.free[px] = False
        special(0, "pixel0"); special(N - 1, "pixelN1")
        for t in sorted(set(tile_of[allowed]))[:3]:                  # all eight pixels of a thread's column: the longest fp32 chain
            for lane in (0, 63, 255):
                for j in range(CHAIN):
                    special(t * TILE + lane + 256 * j, "column8")
        if lone_tile is not None:
            special(min(N, (lone_tile + 1) * TILE) - 1, "tile_last")
        B.index_edges(B.take(counts["index_edges"], allowed), (np.array(sp, np.int64), kinds))
    for fam in ("cancel", "zero_normal", "normal_angle", "distance", "ratio", "chi2_edge", "omega_range", "empty_none", "empty_rejected", "class_edge"):
        n = counts.get(fam, 0)
        if not n:
            continue
        if fam == "cancel":
            for delta, k in ((1, n - n // 2), (256, n // 2)):
                if delta < cols and k:
                    pix = B.take(k, allowed, pair_delta=delta)
                    if len(pix):
                        B.put("cancel", B.cancel(pix, delta))
        elif fam == "empty_none":
            B.empty_none(B.take(n, allowed))
        else:
            pix = B.take(n, allowed)
            B.put("empty" if fam == "empty_rejected" else fam, getattr(B, fam)(pix))
    clouds, index = {}, {}
    for side in ("ref", "cur"):
        rs = B.recs[side]
        cat = {k: (np.concatenate([r[k] for r in rs]) if rs else np.zeros((0,) + {"pos": (3,), "nrm": (3,), "Op": (3, 3), "On": (3, 3)}.get(k, ()), np.float64)) for k in
               ("pix", "pos", "nrm", "curv", "Op", "On", "visible")}
        n = len(cat["pix"])
        perm = rng.permutation(n)
        cat = {k: v[perm] for k, v in cat.items()}
        pos, nrm = cat["pos"], cat["nrm"]
        key = pos[:, 2].copy()                                          # depth in the current frame (the layout)
        if side == "ref" and not exact:
            pos = pos @ G[:3, :3].T + G[:3, 3]; nrm = nrm @ G[:3, :3].T
        pts = np.ones((n, 4), F32); pts[:, :3] = pos.astype(F32)
        nr = np.zeros((n, 4), F32); nr[:, :3] = nrm.astype(F32)
        def m16(o):
            M = np.zeros((n, 4, 4), F32); M[:, :3, :3] = o
            return M.transpose(0, 2, 1).reshape(n, 16).copy()          # column-major 4x4
        clouds[side] = dict(points=pts, normals=nr, curvature=cat["curv"].astype(F32), omega_p=m16(cat["Op"]), omega_n=m16(cat["On"]))
        index[side] = _zbuffer(cat["pix"].astype(np.int64), key, cat["visible"].astype(bool), N).reshape(rows, cols)
    T = G.astype(F32); T[3] = (0, 0, 0, 1)
    return Case(name=name, rows=rows, cols=cols, K=K, guess=T, guess_name=guess if isinstance(guess, str) else name, params=p, ref=clouds["ref"], cur=clouds["cur"],
                family=B.family, sub=B.sub, expect=B.expect, ref_index=index["ref"], cur_index=index["cur"], cls_thr=cls_thr)


# ---------------------------------------------------------------------------------------------------------------- the case sets
_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


SMALL_SIZES = {"zero_normal": (17, 65), "normal_angle": (64, 32), "distance": (3, 683), "ratio": (64, 32), "chi2_edge": (17, 65), "omega_range": (3, 683),
               "cancel": (64, 32), "index_edges": (3, 683)}
SMALL_COUNTS = {"zero_normal": 360, "normal_angle": 660, "distance": 660, "ratio": 800, "chi2_edge": 660, "omega_range": 600, "cancel": 150, "index_edges": 400}


def family_case(fam, guess="identity"):
    """one family alone on a small image (one tile; 2049 pixels: a second tile of one pixel; one partial tile)"""
    def mk():
        rows, cols = SMALL_SIZES[fam]
        params = {"inlier_normal_angular_threshold": 0.0} if fam == "zero_normal" else None
        return make_case(f"{fam}/{guess}", rows, cols, guess, {fam: SMALL_COUNTS[fam]}, seed=1000 + 17 * FAMILIES.index(fam) + sorted(GUESSES).index(guess), params=params)
    return _cached(("family", fam, guess), mk)


def empty_case(kind, guess="identity", rows=17, cols=65):
    key = guess if isinstance(guess, str) else None
    def mk():
        return make_case(f"empty_{kind}/{key}", rows, cols, guess, {f"empty_{kind}": 300}, seed=77)
    return _cached(("empty", kind, key, rows, cols), mk) if key else mk()


MIXED = {fam: 700 for fam in ("zero_normal", "normal_angle", "distance", "ratio", "chi2_edge", "omega_range")}
MIXED.update(cancel=300, index_edges=500)
LARGE_SIZES = ((480, 640), (512, 640), (513, 640))


def mixed_case(rows, cols, guess="identity", tiles=None, lone_tile=None):
    """every family in one pair.  At the large sizes the candidates sit in tiles 0, 3, 156 .. the last one (reduce_partials takes 160 records per
    trip: tile 159 is the last record of the first trip, tile 160 the only record of the second) and tile 7 holds its last pixel only."""
    def mk():
        nt = (rows * cols + TILE - 1) // TILE
        t, lone = tiles, lone_tile
        if nt > 100 and t is None:
            t = sorted({0, 3, nt - 1} | {k for k in range(156, 161) if k < nt} | ({149} if nt == 150 else set()))
            lone = 7
        scale = 1.0 if nt > 1 else 0.25
        return make_case(f"mixed{rows}x{cols}/{guess}", rows, cols, guess, {k: max(50, int(v * scale)) for k, v in MIXED.items()}, seed=500 + rows + cols, tiles=t, lone_tile=lone)
    return _cached(("mixed", rows, cols, guess, None if tiles is None else tuple(tiles), lone_tile), mk)


def cpu_case_set():
    """the cases the CPU test holds to its coverage conditions: every family alone under the three guesses, the mixed pairs at every size"""
    out = [family_case(f, g) for f in SMALL_SIZES for g in GUESSES]
    out += [empty_case("none"), empty_case("rejected"), empty_case("none", "moderate"), empty_case("rejected", "small")]
    out += [mixed_case(r, c) for r, c in ((64, 32), (3, 683), (17, 65)) + LARGE_SIZES] + [mixed_case(480, 640, "moderate")]
    return out


# ---------------------------------------------------------------------------------------------------------------- the converter-form case sets
CLASS_EDGE_SIZES = ((17, 65), (64, 32))
CLASS_THRESHOLDS = (0.02, 0.01, 0.03)            # the shipped default = flat_curvature_threshold; below and above it
CONVERTER_MIXED_SIZES = ((64, 32), (3, 683), (17, 65), (480, 640))


def class_edge_case(rows, cols, guess="identity", cls_thr=0.02):
    """class_edge alone: 900 pixels of 1105 (a partial tile) or of 2048 (one tile)"""
    def mk():
        return make_case(f"class_edge{rows}x{cols}/{guess}/{cls_thr:g}", rows, cols, guess, {"class_edge": 900},
                         seed=3000 + rows + 7 * sorted(GUESSES).index(guess) + int(round(cls_thr * 1000)), cls_thr=cls_thr)
    return _cached(("class_edge", rows, cols, guess, cls_thr), mk)


def class_edge_cases():
    return [class_edge_case(r, c, g, t) for r, c in CLASS_EDGE_SIZES for g in GUESSES for t in CLASS_THRESHOLDS]


def converter_form_cases():
    """(case, cls_thr, table name) of every case run in the converter's form: the x 3 threshold, x 2 table product on the class_edge cases and on
    one mixed case per size; the existing family cases under (0.02, rotated)"""
    out = [(c, c.cls_thr, t) for c in class_edge_cases() for t in ("shipped", "rotated")]
    out += [(mixed_case(r, c), thr, t) for r, c in CONVERTER_MIXED_SIZES for thr in CLASS_THRESHOLDS for t in ("shipped", "rotated")]
    out += [(family_case(f, g), 0.02, "rotated") for f in SMALL_SIZES for g in GUESSES]
    return out


# ---------------------------------------------------------------------------------------------------------------- both sides of a comparison
UPPER_LOWER = [(r + 4 * q, q + 4 * r) for r in range(3) for q in range(3) if r < q]      # column-major 4x4: (upper entry, its mirror)


def arrays_for(cloud, storage):
    """sym6 keeps the upper triangle of Omega_p and mirrors it: the oracle gets the mirrored matrices (as tests/test_omega_sym6.py compares)"""
    if storage != "sym6":
        return cloud
    c = dict(cloud); op = cloud["omega_p"].copy()
    for up, lo in UPPER_LOWER:
        op[:, lo] = op[:, up]
    c["omega_p"] = op
    return c


def oracle_clouds(O, case, storage="exact9"):
    r, c = arrays_for(case.ref, storage), arrays_for(case.cur, storage)
    mk = lambda a: O.Cloud.from_arrays(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])
    return mk(r), mk(c), r, c


def oracle_params(O, case, guess=None, **over):
    p = dict(case.params); p.update(over)
    return O.aligner_params(case.rows, case.cols, K=case.K, initial_guess=case.guess if guess is None else guess, accumulate_fp64=1, **p)


def gpu_aligner(ctx, case, **over):
    from g2o_frontend_amd import api
    p = dict(case.params); p.update(over)
    K = case.K
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]); proj.setMinDistance(p["min_distance"]); proj.setMaxDistance(p["max_distance"])
    proj.setImageSize(case.rows, case.cols)
    f = api.CorrespondenceFinder()
    f.setInlierDistanceThreshold(p["inlier_distance_threshold"]); f.setInlierNormalAngularThreshold(p["inlier_normal_angular_threshold"])
    f.setFlatCurvatureThreshold(p["flat_curvature_threshold"]); f.setInlierCurvatureRatioThreshold(p["inlier_curvature_ratio_threshold"])
    f.setImageSize(case.rows, case.cols)
    lin = api.Linearizer(); lin.setInlierMaxChi2(p["inlier_max_chi2"]); lin.setRobustKernel(p["robust_kernel"])
    a = api.Aligner(ctx)
    a.setProjector(proj); a.setLinearizer(lin); a.setCorrespondenceFinder(f)
    a.setOuterIterations(p["outer_iterations"]); a.setInnerIterations(p["inner_iterations"])
    a.setInitialGuess(case.guess)
    return a


def gpu_clouds(ctx, case):
    from g2o_frontend_amd import api
    out = []
    for a in (case.ref, case.cur):
        c = api.Cloud(ctx, max(1, len(a["points"])))
        c.upload(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])
        out.append(c)
    return out


def hb_bar(Habs, babs, oH, ob, chain):
    """per-entry bar of a GPU H / b against the oracle's float64-accumulated one: a term passes through at most `chain` sequential fp32
    additions in its thread and the 6 levels of the wave tree before the sums turn to double, each addition off by at most 2^-24 of the
    partial sum, itself at most the sum of the magnitudes; the oracle's own rounding of the result to float adds 2^-24 |o|"""
    u = 2.0 ** -24
    return (chain + 6) * u * Habs + u * np.abs(oH), (chain + 6) * u * babs + u * np.abs(ob)


def step_distance(O, M, case, ra, ca, oref, ocur, **over):
    """|oracle's fp32 step - the model's float64 step| (max over the 4x4) for one iteration from the case's guess"""
    p = dict(case.params); p.update(over)
    ap = oracle_params(O, case, **over)
    o = O.align(ap, oref, ocur, images=True)
    Tinv = O.iso_inverse(case.guess)
    corr, _ = M.correspondences(ra, ca, o["ref_index"], o["cur_index"], Tinv, p["inlier_normal_angular_threshold"], p["inlier_distance_threshold"],
                                p["flat_curvature_threshold"], p["inlier_curvature_ratio_threshold"])
    mc = p["inlier_max_chi2"]
    if not p["robust_kernel"]:        # the inlier decision is an fp32 comparison (a term AT the threshold counts): taken from the fp32 local errors
        corr = corr[~(M.local_error_f32(ra, ca, corr, Tinv) > F32(mc))]; mc = np.inf
    H, b, _, _ = M.linearize(ra, ca, corr, Tinv, mc, bool(p["robust_kernel"]))
    dx = np.linalg.solve(H + 1001.0 * np.eye(6), -b)
    Tn = O.v2t(O.t2v(O.iso_inverse(O.iso_mul(O.v2t(dx.astype(F32)), Tinv))))
    return float(np.abs(o["T"].astype(np.float64) - Tn).max()), o
