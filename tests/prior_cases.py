"""Injected (invT, prior) items for the SE(3) prior terms of Aligner::align (pwn_core/se3_prior.cpp:8-71, aligner.cpp:96-108), by family: what
tests/test_prior_terms_cpu.py holds to its claims on the CPU (pwn_hip_prior_terms against the float64 model) and tests/test_gpu_prior_terms.py
feeds to the device kernel (pwn_hip_debug_prior_terms_eval).

invT is Linearizer::_T of an inner iteration, [4, 4] float32, last row 0 0 0 1.  A prior is (kind, mean, referenceTransform, information) as
Aligner.addRelativePrior / addAbsolutePrior store it: kind 0 = SE3RelativePrior, 1 = SE3AbsolutePrior; mean and referenceTransform [4, 4] float32,
information [6, 6] float32 (row-indexed).  The error of a prior is e = t2v(X), X = invT * [referenceTransform^-1 *] mean; every family is built
from the X it wants: mean = referenceTransform * invT^-1 * X in float64, rounded once.

Outcome classes (outcome()):
  "finite"     valid, every word finite
  "nonfinite"  valid, NaNs in the terms.  A mean that holds a NaN or an infinity makes every difference of the numeric Jacobians NaN (inf - inf);
               gauss_jordan_inverse refuses a pivot that EQUALS zero, and a NaN does not, so the elimination runs and the terms are NaN
  "refused"    valid = 0, the terms are zeros: the inverse of Jz was refused.  A mean whose rotation block is zero does that: moving the mean
               along a translation then leaves X as it is, the first column of Jz is exactly zero, and so is the first pivot

Comparison rule (words_equal): bit equality per word, except that two NaNs are equal whatever their sign and payload."""
import zlib

import numpy as np

# the reference transforms tests/test_priors.py uses
_REFT = (np.array([0.02, 0.01, -0.01, 0.0, 0.01, 0.0]), np.array([0.05, -0.02, 0.01, 0.01, 0.0, -0.01]))


def _v2t64(v):
    from numpy_reference_model import _v2t
    return _v2t(np.asarray(v, np.float64))


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _iso(R, t):
    X = np.eye(4); X[:3, :3] = R; X[:3, 3] = t
    return X


def _invT(rng):
    """the inverse of a pose a tracker meets: up to 0.3 m, up to ~7 degrees"""
    T = _v2t64(np.concatenate([rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.06, 0.06, 3)]))
    return np.linalg.inv(T)


def _item(rng, kind, X, info, invT=None):
    """(invT, prior) with invT * [reft^-1 *] mean = X up to the one rounding of mean"""
    invT = _invT(rng) if invT is None else invT
    reft = _v2t64(_REFT[rng.integers(0, 2)]) if kind == 1 else np.eye(4)
    mean = reft @ np.linalg.inv(invT) @ X
    return invT.astype(np.float32), (kind, mean.astype(np.float32), reft.astype(np.float32), np.asarray(info, np.float32))


def _info_diag(scale):
    return lambda rng: np.diag(scale * rng.uniform(0.5, 2.0, 6))


def _info_full(rng):
    A = rng.normal(size=(6, 6)) * np.array([600, 600, 600, 1400, 1400, 1400])
    return A @ A.T


def _info_zero(rng):
    return np.zeros((6, 6))


def _info_rank1(rng):
    a = rng.normal(size=6) * 1e3
    return np.outer(a, a)


INFORMATION = {"diag_1e-3": _info_diag(1e-3), "diag_1": _info_diag(1.0), "diag_1e3": _info_diag(1e3), "diag_1e6": _info_diag(1e6),
               "diag_1e9": _info_diag(1e9), "diag_1e12": _info_diag(1e12), "full": _info_full, "zero": _info_zero, "rank1": _info_rank1}
_INFO_NAMES = list(INFORMATION)


def _motion(size_t, size_q):
    """X = a motion of that size (translation in metres, vector part of the quaternion)"""
    def fam(rng, kind, info):
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        return _item(rng, kind, _v2t64(np.concatenate([size_t * d, size_q * a])), INFORMATION[info](rng))
    return fam


def _branch(which):
    """X's rotation takes branch `which` of t2v's quaternion extraction: 0 = trace > 0 (60 .. 100 degrees about any axis), 1 + i = trace <= 0
    with diagonal entry i the largest (150 .. 175 degrees about an axis near e_i)"""
    def fam(rng, kind, info):
        if which == 0:
            R = _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(60, 100)))
        else:
            axis = np.eye(3)[which - 1] + rng.uniform(-0.2, 0.2, 3)
            R = _rotation(axis, np.deg2rad(rng.uniform(150, 175)))
        return _item(rng, kind, _iso(R, rng.uniform(-0.3, 0.3, 3)), INFORMATION[info](rng))
    return fam


def _near_pi(rng, kind, info):
    R = _rotation(rng.normal(size=3), np.pi - 10.0 ** rng.uniform(-6, -3))
    return _item(rng, kind, _iso(R, rng.uniform(-0.3, 0.3, 3)), INFORMATION[info](rng))


def _nonfinite(rng, kind, info):
    invT, (k, mean, reft, om) = _motion(1e-3, 1e-3)(rng, kind, info)
    bad = [np.nan, np.inf, -np.inf][rng.integers(0, 3)]
    r, c = (rng.integers(0, 3), 3) if rng.integers(0, 2) else (rng.integers(0, 3), rng.integers(0, 3))      # a translation or a rotation entry
    mean = mean.copy(); mean[r, c] = bad
    return invT, (k, mean, reft, om)


def _refused(rng, kind, info):
    invT, (k, mean, reft, om) = _motion(1e-3, 1e-3)(rng, kind, info)
    mean = mean.copy(); mean[:3, :3] = 0.0
    return invT, (k, mean, reft, om)


# family -> (generator(rng, kind, information name), outcome class (None: no claim), compared against the float64 model: "Hb" both terms, "H" Hp only, None)
#   "H": the error e is at or below what fp32 leaves of it (the products behind X round at 6e-8), so bp = J^T Omega' e is compared absolutely
#   None: the numeric Jacobians difference a t2v whose quaternion sits at w ~ 0 (near pi), or there is nothing to compare (refused, nonfinite)
FAMILIES = {
    "identity": (_motion(0.0, 0.0), "finite", "H"),
    "motion_1e-7": (_motion(1e-7, 1e-7), "finite", "H"),
    "motion_1e-3": (_motion(1e-3, 1e-3), "finite", "Hb"),
    "motion_0.3m_6deg": (_motion(0.3, np.sin(np.deg2rad(3.0))), "finite", "Hb"),
    "branch_trace": (_branch(0), "finite", "Hb"),
    "branch_x": (_branch(1), "finite", "Hb"),
    "branch_y": (_branch(2), "finite", "Hb"),
    "branch_z": (_branch(3), "finite", "Hb"),
    "near_pi": (_near_pi, None, None),           # finite or refused: about half of these Jz lose a column to the sign fix of t2v at w ~ 0
    "nonfinite_mean": (_nonfinite, "nonfinite", None),
    "refused": (_refused, "refused", None),
}
BRANCH_OF = {"identity": 0, "motion_1e-7": 0, "motion_1e-3": 0, "motion_0.3m_6deg": 0, "branch_trace": 0, "branch_x": 1, "branch_y": 2, "branch_z": 3}


def items(family, per_cell=4, seed=0):
    """the items of a family: every kind x every information matrix x per_cell draws -> list of (invT, prior, information name)"""
    rng = np.random.default_rng([seed, zlib.crc32(family.encode())])
    gen = FAMILIES[family][0]
    out = []
    for kind in (0, 1):
        for info in INFORMATION:
            for _ in range(per_cell):
                invT, prior = gen(rng, kind, info)
                out.append((invT, prior, info))
    return out


def all_items(per_cell=14, seed=0):
    """every family: list of (family, invT, prior, information name); 11 x 2 x 9 x per_cell items"""
    return [(f,) + it for f in FAMILIES for it in items(f, per_cell, seed)]


def lists(k, n, seed=0):
    """n pairs with k priors each (k = 0 .. 3), drawn from the finite families, all at the pair's one invT: [(invT, [prior, ...])]"""
    rng = np.random.default_rng([seed, 77, k])
    fams = [f for f, (_, cls, _) in FAMILIES.items() if cls == "finite"]
    out = []
    for _ in range(n):
        invT = _invT(rng)
        priors = []
        for _ in range(k):
            fam = fams[rng.integers(0, len(fams))]
            gen = FAMILIES[fam][0]
            # the generator's own invT is dropped: at the pair's invT the prior's error is the family's motion plus the difference of the two
            # poses (at most 0.6 m, ~14 degrees) -- any pairing is an input
            _, (kind, mean, reft, om) = gen(rng, int(rng.integers(0, 2)), _INFO_NAMES[rng.integers(0, len(_INFO_NAMES))])
            priors.append((kind, mean, reft, om))
        out.append((invT.astype(np.float32), priors))
    return out


# ---- what the tests share -------------------------------------------------------------------------------------------------------------------
def prior_struct(prior):
    """the pwn_hip_prior of a prior tuple"""
    from g2o_frontend_amd import _lib
    kind, mean, reft, info = prior
    q = _lib.Prior()
    q.kind = int(kind)
    q.mean[:] = np.asarray(mean, np.float32).T.reshape(-1).tolist()
    q.reference_transform[:] = np.asarray(reft, np.float32).T.reshape(-1).tolist()
    q.information[:] = np.asarray(info, np.float32).T.reshape(-1).tolist()
    return q


def host_terms(invT, prior):
    """pwn_hip_prior_terms: the record [44] as the device writes it (uint32 words: Hp[36] column-major, bp[6], valid, 0)"""
    import ctypes as C
    from g2o_frontend_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    L.pwn_hip_prior_terms.restype = None
    L.pwn_hip_prior_terms.argtypes = [C.c_void_p] * 4 + [C.POINTER(C.c_int)]
    it = np.ascontiguousarray(np.asarray(invT, np.float32).T)
    rec = np.zeros(44, np.float32); valid = C.c_int(-1)
    q = prior_struct(prior)
    L.pwn_hip_prior_terms(it.ctypes.data, C.byref(q), rec.ctypes.data, rec[36:].ctypes.data, C.byref(valid))
    w = rec.view(np.uint32).copy(); w[42] = valid.value; w[43] = 0
    return w


def record_parts(words):
    """(Hp [6, 6] row-indexed, bp [6], valid) of a 44-word record"""
    w = np.ascontiguousarray(words, np.uint32)
    f = w.view(np.float32)
    return f[:36].reshape(6, 6).T.copy(), f[36:42].copy(), int(w[42])


def outcome(words):
    Hp, bp, valid = record_parts(words)
    if not valid:
        return "refused"
    return "finite" if np.all(np.isfinite(Hp)) and np.all(np.isfinite(bp)) else "nonfinite"


def words_equal(a, b):
    """the comparison rule, per word: bool array.  The last two words (valid, 0) compare as integers."""
    a = np.ascontiguousarray(a, np.uint32); b = np.ascontiguousarray(b, np.uint32)
    fa, fb = a.view(np.float32), b.view(np.float32)
    eq = a == b
    nan = np.isnan(fa) & np.isnan(fb)
    nan.reshape(-1, 44)[:, 42:] = False
    return eq | nan


def error_rotation(invT, prior):
    """X's rotation block as the text computes it (fp32, the library's iso_mul / iso_inverse): [3, 3] float32"""
    import ctypes as C
    from g2o_frontend_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for f in ("pwn_hip_iso_mul", "pwn_hip_iso_inverse"):
        getattr(L, f).restype = None
    kind, mean, reft, _ = prior
    cm = lambda M: np.ascontiguousarray(np.asarray(M, np.float32).T)
    out = np.zeros(16, np.float32)
    a = cm(invT)
    if kind == 1:
        ir = np.zeros(16, np.float32); r = cm(reft)
        L.pwn_hip_iso_inverse(C.c_void_p(r.ctypes.data), C.c_void_p(ir.ctypes.data))
        t = np.zeros(16, np.float32)
        L.pwn_hip_iso_mul(C.c_void_p(a.ctypes.data), C.c_void_p(ir.ctypes.data), C.c_void_p(t.ctypes.data))
        a = t
    m = cm(mean)
    L.pwn_hip_iso_mul(C.c_void_p(a.ctypes.data), C.c_void_p(m.ctypes.data), C.c_void_p(out.ctypes.data))
    return out.reshape(4, 4).T[:3, :3].copy()


def t2v_branch(R):
    """the branch of mat2quat (bm_se3.h:25-35, Eigen's Quaternionf(Matrix3f)) a rotation block takes: 0 = trace > 0, 1 + i = diagonal i largest"""
    R = np.asarray(R, np.float32)
    if np.float32(np.float32(R[0, 0] + R[1, 1]) + R[2, 2]) > 0:
        return 0
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > (R[0, 0] if i == 0 else R[1, 1]):
        i = 2
    return 1 + i
