"""Inputs and a float64 model for the alignment loop WITH SE(3) priors (Aligner::align, aligner.cpp:49-125 with :96-108) on the injected clouds
of tests/align_clouds.py: the cases, the prior lists, model_step and the wrong loops a kernel could run in its place.  A helper module of
tests/test_prior_steps_cpu.py (which holds the conditions below from the reference side) and tests/test_gpu_prior_steps.py (which holds the
device loop to the oracle); nothing here needs a GPU and nothing here is a test.

Cases: pairs at one size (17 x 65, one partial tile) with the shared PARAMS so that they go into one batch, from the modest-information
families (`cancel`, `index_edges`) under the three GUESSES -- on chi2_edge / omega_range clouds H is so large that a prior of INFO moves
nothing -- plus one 64 x 32 and one 3 x 683 case for the single-pair parts.

Prior lists (LISTS), per case, each mean a few centimetres and a fraction of a degree off the case's guess: none; one relative; one absolute
(with a reference transform); absolute + relative (the tracker's order); three; three with a REFUSED prior (a mean whose rotation block is
zero: the inverse of Jz is refused, se3_prior.cpp:50, tests/prior_cases.py) in the middle; three with the refused prior in front.

model_step is the loop in float64: correspondences by the reference's fp32 tests (numpy_reference_model.correspondences), then per inner
iteration M.linearize at the current invT + 1001 I + M.prior_terms of each non-refused prior in list order, solve, invT <- v2t(dx) invT; at
the end of an outer iteration T = v2t(t2v(invT^-1)); a further outer iteration re-projects the reference cloud at that T.

VARIANTS are the wrong loops: "none" (priors dropped), "stale_inner" (the terms of inner iteration k > 0 at the first one's invT),
"first_inner_only" (terms dropped after the first inner iteration), "stale_outer" (the terms of outer iteration o > 0 at the invT the previous
outer iteration used), "neighbour" (the next pair's list), "in_statistics" (the statistics H with the terms added).
"""
from __future__ import annotations

import zlib

import numpy as np

import align_clouds as A
import flat_clouds as FC
import numpy_reference_model as M

F32 = np.float32
INFO = (np.diag([4e5, 4e5, 4e5, 2e6, 2e6, 2e6]) + 1e4).astype(F32)      # tests/test_priors.py
SIZE = (17, 65)
LISTS = ("none", "relative", "absolute", "absolute+relative", "three", "refused_middle", "refused_front")
VARIANTS = ("none", "stale_inner", "first_inner_only", "stale_outer", "neighbour", "in_statistics")
FORMS = ("uploaded", "converter")
CONVERTER_FORM = (0.02, "rotated")            # threshold and class table of the converter-form clouds (tests/test_gpu_converter_form.py)
REFT = (np.array([0.02, 0.01, -0.01, 0.0, 0.01, 0.0]), np.array([0.05, -0.02, 0.01, 0.01, 0.0, -0.01]))      # tests/test_priors.py

# (name, guess, counts, seed, power of ten on INFO): nine pairs for the batch -- seven lists, a second pair without priors, one more
_BATCH = (("cancel/a", "identity", {"cancel": 150, "index_edges": 60}, 11, 0),
          ("cancel/b", "small", {"cancel": 150, "index_edges": 60}, 12, 0),
          ("cancel/c", "moderate", {"cancel": 150, "index_edges": 60}, 13, 0),
          ("edges/a", "small", {"cancel": 60, "index_edges": 300}, 14, 0),
          ("edges/b", "moderate", {"cancel": 60, "index_edges": 300}, 15, 0),
          ("edges/c", "identity", {"cancel": 60, "index_edges": 300}, 16, 0),
          ("cancel/d", "moderate", {"cancel": 200, "index_edges": 100}, 17, 0),
          ("cancel/e", "identity", {"cancel": 100, "index_edges": 150}, 18, 0),
          ("edges/d", "small", {"cancel": 120, "index_edges": 200}, 19, 0))
_SINGLE = (("single64x32", 64, 32, "small", {"cancel": 150, "index_edges": 60}, 21, 0),
           ("single3x683", 3, 683, "moderate", {"cancel": 150, "index_edges": 60}, 22, 0))
N_CASES = len(_BATCH) + len(_SINGLE)
_cache = {}


def _case(name, rows, cols, guess, counts, seed, power):
    key = ("case", name)
    if key not in _cache:
        c = A.make_case(f"prior/{name}/{guess}", rows, cols, guess, counts, seed=seed)
        c.prior_scale = 10.0 ** power
        _cache[key] = c
    return _cache[key]


def batch_cases():
    """the 17 x 65 pairs, in the batch's base order; pair i carries list LISTS[BATCH_LISTS[i]]"""
    return [_case(n, SIZE[0], SIZE[1], g, c, s, p) for n, g, c, s, p in _BATCH]


def single_cases():
    return [_case(*t) for t in _SINGLE]


def all_cases():
    return batch_cases() + single_cases()


BATCH_LISTS = (0, 1, 2, 3, 4, 5, 6, 0, 1)
# two orders of the nine pairs in sub-batches of four (4 + 4 + 1): in the first a pair without priors (0) opens a sub-batch and the other one
# (7) is a sub-batch of its own -- plain k_solve_update beside k_solve_update_priors; in the second they close their sub-batches
ORDERS = ((0, 1, 2, 3, 4, 5, 6, 8, 7), (1, 2, 3, 0, 4, 5, 6, 7, 8))


OUTERS = (2, 3)                               # outer_iterations of the one-call part; 3 on OUTER3_CASE only
OUTER3_CASE = 1


def part_a():
    """what the single-call part runs, in both files: (case, list name, inner_iterations, parameter overrides) -- every case x every list x inner
    1 and 2 with the robust kernel, and without it on the first case"""
    out = [(c, name, inner, {}) for c in all_cases() for name in LISTS for inner in (1, 2)]
    out += [(batch_cases()[0], name, inner, {"robust_kernel": 0}) for name in LISTS for inner in (1, 2)]
    return out


def part_b():
    """the candidates of the one-call outer_iterations > 1 part: (case, list name, inner, outer); two lists per case, every list with a prior
    on some case.  A candidate runs where outer_fit says so."""
    out = []
    for i, c in enumerate(all_cases()):
        for name in (LISTS[1 + i % 6], LISTS[1 + (i + 3) % 6]):
            for inner in (1, 2):
                out += [(c, name, inner, outer) for outer in OUTERS if outer == 2 or i == OUTER3_CASE]
    return out


def batch_lists(cases=None):
    """the list of every pair of the batch, in the base order"""
    cases = batch_cases() if cases is None else cases
    return [prior_list(c, BATCH_LISTS[i]) for i, c in enumerate(cases)]


# ---------------------------------------------------------------------------------------------------------------- float64 SE(3)
def inv64(T):
    T = np.asarray(T, np.float64)
    out = np.eye(4); out[:3, :3] = T[:3, :3].T; out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def inverse_f32(T):
    """Isometry3f::inverse() in fp32 with left-to-right inner products: the transform the finder is handed"""
    T = np.asarray(T, F32)
    Rt = T[:3, :3].T.copy()
    out = np.eye(4, dtype=F32); out[:3, :3] = Rt; out[:3, 3:4] = M._mm3(-Rt, T[:3, 3:4])
    return out


# ---------------------------------------------------------------------------------------------------------------- the prior lists
def is_refused(prior):
    """a mean whose rotation block is zero: the first column of Jz is exactly zero, its inverse is refused and the prior adds nothing"""
    return not np.any(np.asarray(prior[1])[:3, :3])


def prior_list(case, which):
    """list `which` (a name of LISTS or its number) of the case: tuples (kind, mean, referenceTransform, information) as
    Aligner.addRelativePrior / addAbsolutePrior store them"""
    which = LISTS[which] if isinstance(which, int) else which
    key = ("list", case.name, which)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    P = np.asarray(case.guess, np.float64)
    info = (INFO.astype(np.float64) * case.prior_scale)

    def offset():     # 1 .. 3 cm per axis, 0.002 .. 0.008 in the quaternion's vector part (0.2 .. 0.9 degrees per axis)
        return M._v2t(np.concatenate([rng.choice([-1, 1], 3) * rng.uniform(0.01, 0.03, 3), rng.choice([-1, 1], 3) * rng.uniform(0.002, 0.008, 3)]))

    def rel(scale=1.0):
        return (0, (P @ offset()).astype(F32), np.eye(4, dtype=F32), (info * scale).astype(F32))

    def ab(k, scale=0.5):
        reft = M._v2t(REFT[k])
        return (1, (reft @ P @ offset()).astype(F32), reft.astype(F32), (info * scale).astype(F32))

    def refused(kind):
        k, mean, reft, om = rel() if kind == 0 else ab(1)
        mean = mean.copy(); mean[:3, :3] = 0.0
        return (k, mean, reft, om)

    # every list draws all its offsets, whichever it is, so that the lists of one case do not share means
    draws = {"none": [], "relative": [rel()], "absolute": [ab(0)], "absolute+relative": [ab(1), rel()], "three": [rel(), ab(0), rel(0.25)],
             "refused_middle": [rel(), refused(1), ab(0)], "refused_front": [refused(0), ab(1), rel()]}
    for k, v in draws.items():
        _cache[("list", case.name, k)] = v
    return _cache[key]


def without_refused(plist):
    return [q for q in plist if not is_refused(q)]


# ---------------------------------------------------------------------------------------------------------------- clouds of a case, both forms
def arrays(case, form="uploaded", storage="exact9"):
    """(reference, current) arrays as the oracle and the model get them: the case's own (uploaded form) or with Omega_n by the class rule of the
    converter's form"""
    if form == "uploaded":
        return A.arrays_for(case.ref, storage), A.arrays_for(case.cur, storage)
    thr, tname = CONVERTER_FORM
    return tuple(FC.oracle_arrays(case, storage, FC.TABLES[tname], thr))


def oracle_clouds(O, arrs):
    return tuple(O.Cloud.from_arrays(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"]) for a in arrs)


def oracle_step(O, case, oclouds, plist, inner=1, outer=1, images=True, **over):
    """the oracle's align() from the case's guess with the list added in its order (oracle.add_prior); the oracle's list is left empty"""
    ap = A.oracle_params(O, case, inner_iterations=inner, outer_iterations=outer, **over)
    O.clear_priors()
    try:
        for kind, mean, reft, info in plist:
            O.add_prior(kind, mean, info, reference_transform=reft if kind == 1 else None)
        return O.align(ap, oclouds[0], oclouds[1], images=images)
    finally:
        O.clear_priors()


# ---------------------------------------------------------------------------------------------------------------- the model and the wrong loops
def _finder_args(p):
    return (p["inlier_normal_angular_threshold"], p["inlier_distance_threshold"], p["flat_curvature_threshold"], p["inlier_curvature_ratio_threshold"])


def _terms(plist, invT):
    Hp, bp = np.zeros((6, 6)), np.zeros(6)
    for kind, mean, reft, info in plist:                      # in list order
        if is_refused((kind, mean, reft, info)):
            continue
        h, b = M.prior_terms(kind, mean, info, invT, reft)
        Hp = Hp + h; bp = bp + b
    return Hp, bp


def model_step(case, clouds, index_images, plist, inner, outer=1, variant=None, neighbour=None, **over):
    """the loop in float64 from the case's guess.  clouds = (reference, current) arrays; index_images = (reference, current) index image of the
    first outer iteration (later ones: M.project at the model's own pose); plist = the pair's list; variant: None or a name of VARIANTS
    ("neighbour" takes the list `neighbour`).  Returns dict(T [4, 4] float64, iterations = [dict(K, C, inliers, invT)] per inner iteration of
    every outer one, corr = the last outer iteration's list, ref_index of every outer iteration, stat_H = the H of the statistics pass:
    M.linearize at T^-1 on the last list)."""
    assert variant is None or variant in VARIANTS
    p = dict(case.params); p.update(over)
    ra, ca = clouds
    robust = bool(p["robust_kernel"])
    use = {"none": [], "neighbour": neighbour}.get(variant, plist)
    assert use is not None
    ref_index, cur_index = index_images
    T = np.asarray(case.guess, np.float64)
    its, ref_indices = [], []
    previous = None                                            # the invT of the previous outer iteration's inner iterations
    for o in range(outer):
        T32 = T.astype(F32); T32[3] = (0, 0, 0, 1)
        if o > 0:
            ref_index, _ = M.project(ra["points"][:, :3], M.projector_matrices(case.K, T32)[0], p["min_distance"], p["max_distance"], case.rows, case.cols)
        ref_indices.append(ref_index)
        corr_all, K = M.correspondences(ra, ca, ref_index, cur_index, inverse_f32(T32), *_finder_args(p))
        invT = inv64(T)
        used = []
        for k in range(inner):
            corr, mc = corr_all, p["inlier_max_chi2"]
            if not robust:      # the inlier decision is an fp32 comparison (a term AT the threshold counts): taken from the fp32 local errors
                corr = corr_all[~(M.local_error_f32(ra, ca, corr_all, invT) > F32(mc))]; mc = np.inf
            H, b, _, inl = M.linearize(ra, ca, corr, invT, mc, robust)
            at = invT
            if variant == "stale_inner" and k > 0:
                at = used[0]
            if variant == "stale_outer" and o > 0:
                at = previous[k]
            if variant == "first_inner_only" and k > 0:
                Hp, bp = np.zeros((6, 6)), np.zeros(6)
            else:
                Hp, bp = _terms(use, at)
            its.append(dict(K=K, C=len(corr_all), inliers=inl, invT=invT))
            used.append(invT)
            dx = np.linalg.solve(H + 1001.0 * np.eye(6) + Hp, -(b + bp))
            invT = M._v2t(dx) @ invT
        previous = used
        T = M._v2t(M._t2v(inv64(invT)))
    invT = inv64(T)
    corr, mc = corr_all, p["inlier_max_chi2"]
    if not robust:
        corr = corr_all[~(M.local_error_f32(ra, ca, corr_all, invT) > F32(mc))]; mc = np.inf
    stat_H = M.linearize(ra, ca, corr, invT, mc, robust, abs_sums=True)
    H = stat_H[0]
    if variant == "in_statistics":
        H = H + _terms(use, invT)[0]
    return dict(T=T, iterations=its, corr=corr_all, ref_index=ref_indices, stat_H=H, stat_Habs=stat_H[4])


def distance(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def outer_fit(O, case, form, plist, inner, outer, storage="exact9"):
    """whether the case may enter the one-call outer > 1 part: the oracle's run and the model-led run have equal K, C and inliers in every
    iteration, and M.correspondences of every later outer iteration gives the same list at the oracle's pose as at the model's.  Returns
    (fit, oracle result, model result)."""
    key = ("fit", case.name, form, id(plist), inner, outer, storage)
    if key in _cache:
        return _cache[key]
    arrs = arrays(case, form, storage)
    oc = oracle_clouds(O, arrs)
    o = oracle_step(O, case, oc, plist, inner, outer)
    cur_index = o["cur_index"]
    first = oracle_step(O, case, oc, plist, inner, 1)
    m = model_step(case, arrs, (first["ref_index"], cur_index), plist, inner, outer)
    fit = len(o["iterations"]) == len(m["iterations"]) == inner * outer
    fit = fit and all((a["K"], a["C"], a["inliers"]) == (b["K"], b["C"], b["inliers"]) for a, b in zip(o["iterations"], m["iterations"]))
    p = case.params
    for n in range(1, outer):      # the finder of outer iteration n at the oracle's pose after n iterations against the model's
        To = oracle_step(O, case, oc, plist, inner, n, images=False)["T"]
        ri, _ = M.project(arrs[0]["points"][:, :3], M.projector_matrices(case.K, To)[0], p["min_distance"], p["max_distance"], case.rows, case.cols)
        co, _ = M.correspondences(arrs[0], arrs[1], ri, cur_index, inverse_f32(To), *_finder_args(p))
        mn = model_step(case, arrs, (first["ref_index"], cur_index), plist, inner, n + 1)
        fit = fit and np.array_equal(ri, mn["ref_index"][n]) and np.array_equal(co, mn["corr"])
    _cache[key] = (bool(fit), o, m)
    return _cache[key]
