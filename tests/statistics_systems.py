"""Injected systems (H, T) for Aligner::_computeStatistics (pwn_core/aligner.cpp:152-199), by family: what tests/test_statistics_systems_cpu.py holds
to its claims on the CPU and tests/test_gpu_closure_records.py feeds to the device kernel (pwn_hip_debug_statistics_eval).

H is Linearizer::H() without damping, row-indexed [6, 6] float32 (symmetric); T the final transform, [4, 4] float32.  The statistics add I to H, so a
direction H does not constrain has the eigenvalue 1 exactly: its sigma points (sqrt(6 + 6e-6) long) leave the unit ball of the quaternion chart and
v2t takes the root of a negative number -- the reference produces NaN there, and so must every restatement, in the same words of the result.

Comparison rule (words_equal): bit equality per word, except that two NaNs are equal whatever their sign and payload (x86 and the GPU produce
different default NaNs); a NaN on one side only, or an infinity of the other sign, is a difference."""
import numpy as np

_SCALE = np.array([30, 30, 30, 60, 60, 60], np.float64)


def _small_T(rng):
    from g2o_frontend_amd import synth
    return synth.v2t(np.concatenate([rng.uniform(-0.2, 0.2, 3), rng.uniform(-0.05, 0.05, 3)])).astype(np.float32)


def _J(rng):
    return rng.normal(size=(200, 6)) * _SCALE


def _jtj(J):
    return (J.T @ J).astype(np.float32)


def _rotation(axis, angle):
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _fam_jtj(rng):                    # tests/test_statistics.py::random_system
    return _jtj(_J(rng)), _small_T(rng)


def _fam_jtj_x100(rng):               # H near 1e8: the magnitudes of a VGA pair
    return _jtj(_J(rng) * 10.0), _small_T(rng)


def _fam_jtj_x1e4(rng):
    return _jtj(_J(rng) * 100.0), _small_T(rng)


def _fam_diagonal(rng):               # no off-diagonal entry: the Jacobi loop ends before its first sweep
    return np.diag(np.diag(_jtj(_J(rng)))).astype(np.float32), _small_T(rng)


def _fam_near_pi(rng):                # rotation within 1e-6 ... 1e-1 of pi: t2v with qw -> 0 (the trace <= 0 branches of mat2quat)
    T = np.eye(4)
    T[:3, :3] = _rotation(rng.normal(size=3), np.pi - 10.0 ** rng.uniform(-6, -1))
    T[:3, 3] = rng.uniform(-0.2, 0.2, 3)
    return _jtj(_J(rng)), T.astype(np.float32)


def _zeroed(k):                       # k zeroed columns of a J of scale 1: each an eigenvalue of exactly 1 after + I
    def fam(rng):
        J = rng.normal(size=(200, 6))
        J[:, rng.choice(6, size=k, replace=False)] = 0.0
        return _jtj(J), _small_T(rng)
    return fam


def _fam_dependent(rng):              # a nearly dependent sixth column (relative 1e-4)
    J = rng.normal(size=(200, 6))
    J[:, 5] = J[:, 4] + 1e-4 * J[:, 5]
    return _jtj(J), _small_T(rng)


def _fam_zero(rng):
    return np.zeros((6, 6), np.float32), _small_T(rng)


def _fam_huge(rng):                   # H near 1e18: the covariance underflows and the inverse is refused (omega = 0)
    return _jtj(_J(rng) * 1e7), _small_T(rng)


def _sv(lo, hi):
    """An unconstrained TRANSLATION (eigenvalue exactly 1 after + I, sigma points stay harmless) with the largest eigenvalue in [lo, hi]: the
    pseudo-inverse drops |w| <= FLT_EPSILON * 6 * smax, i.e. the eigenvalue 1 from smax = 1.4e6 on."""
    def fam(rng):
        J = _J(rng)
        J[:, rng.integers(0, 3)] = 0.0
        H = J.T @ J
        H *= rng.uniform(lo, hi) / np.linalg.eigvalsh(H)[-1]
        return H.astype(np.float32), _small_T(rng)
    return fam


def _fam_tiny_offdiag(rng):           # an off-diagonal entry below 1e-30 beside ordinary ones: the rotation (0, 1) of the first sweep is skipped
    H = _jtj(_J(rng))
    H[0, 1] = H[1, 0] = np.float32(10.0 ** rng.uniform(-38, -31) * rng.choice([-1.0, 1.0]))
    return H, _small_T(rng)


def _fam_pivot_swap(rng):
    """A covariance whose entry (3, 0) is larger than its entry (0, 0): a tight translation strongly correlated with a loose rotation, so
    gauss_jordan_inverse swaps rows in its first column.  H = Sigma^-1 - I for that Sigma."""
    std = np.array([1e-3, 1e-3, 1e-3, 3e-2, 3e-2, 3e-2]) * rng.uniform(0.5, 2.0, 6)
    R = np.eye(6)
    R[0, 3] = R[3, 0] = rng.uniform(0.8, 0.95) * rng.choice([-1.0, 1.0])
    Sigma = np.diag(std) @ R @ np.diag(std)
    T = np.eye(4); T[:3, 3] = rng.uniform(-0.2, 0.2, 3)
    return (np.linalg.inv(Sigma) - np.eye(6)).astype(np.float32), T.astype(np.float32)


# family -> (generator, the outcome class most of its systems fall into: "finite", "nonfinite" or "zero" = omega all zero)
FAMILIES = {
    "jtj": (_fam_jtj, "finite"),
    "jtj_x100": (_fam_jtj_x100, "finite"),
    "jtj_x1e4": (_fam_jtj_x1e4, "finite"),
    "diagonal": (_fam_diagonal, "finite"),
    "near_pi": (_fam_near_pi, "finite"),
    "zeroed_1": (_zeroed(1), "finite"),
    "zeroed_2": (_zeroed(2), "nonfinite"),
    "zeroed_3": (_zeroed(3), "nonfinite"),
    "dependent": (_fam_dependent, "nonfinite"),
    "zero": (_fam_zero, "nonfinite"),
    "huge": (_fam_huge, "zero"),
    "sv_kept": (_sv(0.6e6, 1.2e6), None),
    "sv_dropped": (_sv(1.7e6, 3.0e6), None),
    "tiny_offdiag": (_fam_tiny_offdiag, "finite"),
    "pivot_swap": (_fam_pivot_swap, "finite"),
}


def systems(family, n, seed=0):
    """n systems of a family: H [n, 6, 6], T [n, 4, 4], float32"""
    import zlib
    rng = np.random.default_rng([seed, zlib.crc32(family.encode())])
    gen = FAMILIES[family][0]
    H = np.empty((n, 6, 6), np.float32); T = np.empty((n, 4, 4), np.float32)
    for i in range(n):
        H[i], T[i] = gen(rng)
    return H, T


def outcome(words):
    """class of a result (any float array holding omega first): "nonfinite", "zero" (omega all zero) or "finite" """
    w = np.asarray(words, np.float32).reshape(-1)
    if not np.any(w[:36]):
        return "zero"            # the refused inverse; both eigen ratios are then 0 / 0
    return "finite" if np.all(np.isfinite(w)) else "nonfinite"


def oracle_words(oracle, H, T):
    """[44] float32 of one system by the oracle: omega column-major, mean, translational and rotational eigen ratio"""
    s = oracle.compute_statistics(H, T)
    return np.concatenate([s["omega"].T.reshape(-1), s["mean"], np.array([s["translationalEigenRatio"], s["rotationalEigenRatio"]], np.float32)]).astype(np.float32)


def words_equal(a, b):
    """the comparison rule, per word: [k] bool"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def drops_unit_eigenvalue(H):
    """the pseudo-inverse's rule on the exact spectrum of H + I: is the eigenvalue 1 at or below FLT_EPSILON * 6 * smax?"""
    smax = np.linalg.eigvalsh(H.astype(np.float64) + np.eye(6))[-1]
    return 1.0 <= float(np.finfo(np.float32).eps) * 6 * smax


def swaps_rows(omega):
    """Does a Gauss-Jordan elimination with partial pivoting swap rows on the covariance omega is the inverse of?  (float64 re-run of the pivot
    search on omega^-1; omega row-indexed [6, 6], finite and regular)"""
    a = np.linalg.inv(np.asarray(omega, np.float64))
    swapped = False
    for c in range(6):
        piv = c + int(np.argmax(np.abs(a[c:, c])))
        if piv != c:
            a[[c, piv]] = a[[piv, c]]; swapped = True
        a[c] /= a[c, c]
        for r in range(6):
            if r != c:
                a[r] -= a[r, c] * a[c]
    return swapped
