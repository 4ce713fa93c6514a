"""The aligner's fused pass (k_corr_linearize, k_corr_linearize_lat), its list twin (k_linearize_list) and the solve step (k_solve_update) on the
injected clouds of tests/align_clouds.py, uploaded through pwn_hip_cloud_upload (full Omega_n planes), in both Omega_p storages:

  1. the finder on the case's index images equals the oracle's list exactly;
  2. one outer iteration, teacher-forced from the case's guess: images bit for bit, (K, C, inliers) exact, chi2 within CHI2_RTOL, and the H, b,
     error and inliers of the statistics pass against the oracle's Linearizer::update at the GPU's returned T, entry by entry within
         |g - o| <= (chain + 6) 2^-24 sum|term| + 2^-24 |o|
     -- a term passes through at most `chain` sequential fp32 additions in its thread (kPixPerThread = 8: the thread's column of the tile in the
     fused pass, the unrolled loop `for j < kPixPerThread` of k_linearize_list) and the 6 levels of the 64-lane wave tree before the sums turn
     to double; sum|term| is the float64 sum of the magnitudes of the per-correspondence terms (numpy_reference_model.linearize);
  3. the pose after that iteration within max(5e-6, 4 x the oracle's own distance from the float64 step, tests/test_align_clouds_cpu.py);
  4. mat2quat's trace <= 0 branches inside k_solve_update: `empty` cases (dx = 0) under rotations of 125 .. 180 degrees, bitwise against the oracle;
  5. the two kernel shapes: single pairs (latency shape) against batches (throughput shape), result records bitwise equal.
"""
import functools
import sys

import numpy as np
import pytest

import align_clouds as A
import numpy_reference_model as M
from test_align_clouds_cpu import ORACLE_STEP_DISTANCE

pytestmark = pytest.mark.gpu

CHI2_RTOL = 1e-5                                       # tests/test_gpu_parity.py
STEP_BAR = max(5e-6, 4 * ORACLE_STEP_DISTANCE)         # 5e-6: test_gpu_alignment_against_the_numpy_model's bar; 4 x: the other summation order
FUSED_CHAIN = A.CHAIN                                  # kPixPerThread pixels of one thread, added in order to its LDS column
LIST_CHAIN = 8                                         # k_linearize_list: `for (j = 0; j < kPixPerThread; ++j)` adds into the thread's registers
STORAGES = ("exact9", "sym6")
_ctx = {}
_report = {}


@pytest.fixture(scope="module")
def rig():
    from g2o_frontend_amd import api

    def get(storage):
        if storage not in _ctx:
            _ctx[storage] = api.Context(device=0, max_rows=513, max_cols=683, max_batch=8, omega_storage=storage)
        return _ctx[storage]
    yield get
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def uploaded(ctx, case, storage, oracle):
    """the cloud maker of this module: pwn_hip_cloud_upload of the case's arrays (full Omega_n planes), the same arrays for the oracle.
    A maker returns ((reference, current) GPU clouds, (reference, current) oracle clouds, (reference, current) arrays)."""
    oref, ocur, ra, ca = A.oracle_clouds(oracle, case, storage)
    return A.gpu_clouds(ctx, case), (oref, ocur), (ra, ca)


def _pair(rig, oracle, case, storage, maker=uploaded, **over):
    ctx = rig(storage)
    (gref, gcur), (oref, ocur), (ra, ca) = maker(ctx, case, storage, oracle)
    assert gcur.omega_storage() == storage
    al = A.gpu_aligner(ctx, case, **over)
    al.setReferenceCloud(gref); al.setCurrentCloud(gcur)
    return al, (gref, gcur), (oref, ocur, ra, ca), A.oracle_params(oracle, case, **over), dict(case.params, **over)


def _finder_args(p):
    return (p["inlier_normal_angular_threshold"], p["inlier_distance_threshold"], p["flat_curvature_threshold"], p["inlier_curvature_ratio_threshold"])


def _check_hb(tag, g, o, ra, ca, corr, invT, p, chain):
    """H, b of a GPU linearization against the oracle's, entry by entry within the derived bar; returns the worst error as a fraction of its bar"""
    _, _, _, _, Habs, babs = M.linearize(ra, ca, corr, invT, p["inlier_max_chi2"], bool(p["robust_kernel"]), abs_sums=True)
    if not p["robust_kernel"]:      # the inlier set is an fp32 decision: magnitudes over the terms the oracle kept
        keep = ~(M.local_error_f32(ra, ca, corr, invT) > np.float32(p["inlier_max_chi2"]))
        _, _, _, _, Habs, babs = M.linearize(ra, ca, corr[keep], invT, np.inf, False, abs_sums=True)
    barH, barb = A.hb_bar(Habs, babs, o["H"].astype(np.float64), o["b"].astype(np.float64), chain)
    dH = np.abs(g["H"].astype(np.float64) - o["H"]); db = np.abs(g["b"].astype(np.float64) - o["b"])
    frac = max(float((dH / np.maximum(barH, 1e-300)).max()), float((db / np.maximum(barb, 1e-300)).max()))
    print(f"    {tag}: worst H/b error {frac:.3f} of its bar")
    assert (dH <= barH).all(), (tag, "H", np.argwhere(dH > barH).tolist(), float((dH / np.maximum(barH, 1e-300)).max()))
    assert (db <= barb).all(), (tag, "b", np.argwhere(db > barb).tolist(), float((db / np.maximum(barb, 1e-300)).max()))
    return frac


def _chi2_close(g, o):
    return g == 0 if o == 0 else abs(g - o) <= CHI2_RTOL * o


def _check_fused(rig, oracle, case, storage, maker=uploaded, step_bar=STEP_BAR, step_note=ORACLE_STEP_DISTANCE, **over):
    """parts 2 and 3 for one case, on the clouds `maker` makes of it (tests/test_gpu_converter_form.py hands in clouds of the converter's form and
    the pose bar derived for them)"""
    O = oracle
    al, keep, (oref, ocur, ra, ca), ap, p = _pair(rig, O, case, storage, maker, **over)
    g = al.align(images=True, statistics=True)
    o = O.align(ap, oref, ocur, images=True)
    f = al.correspondenceFinder()
    assert np.array_equal(f.referenceIndexImage(), o["ref_index"]) and np.array_equal(f.currentIndexImage(), o["cur_index"]), case.name
    assert np.array_equal(f.referenceDepthImage().view(np.uint32), o["ref_depth"].view(np.uint32)), case.name
    assert np.array_equal(f.currentDepthImage().view(np.uint32), o["cur_depth"].view(np.uint32)), case.name
    assert np.array_equal(o["ref_index"], case.ref_index) and np.array_equal(o["cur_index"], case.cur_index)
    n_it = p["inner_iterations"]
    assert g["iterations"] == n_it == len(o["iterations"])
    i0 = o["iterations"][0]
    assert (int(g["K"][0]), int(g["C"][0]), int(g["iter_inliers"][0])) == (i0["K"], i0["C"], i0["inliers"]), case.name
    assert i0["K"] == int(case.candidates().sum())
    chi2_d = abs(float(g["chi2"][0]) - i0["chi2_fp64"]) / i0["chi2_fp64"] if i0["chi2_fp64"] else abs(float(g["chi2"][0]))
    assert _chi2_close(float(g["chi2"][0]), i0["chi2_fp64"]), (case.name, float(g["chi2"][0]), i0["chi2_fp64"])
    for k in range(1, n_it):
        # a later inner iteration linearizes at each side's own iterate (they differ by the step distance below): the finder's counters stay
        # exact, the robust kernel keeps every correspondence; chi2 is printed (a 5e-6 pose difference moves a millimetre-sized error by 1e-2)
        ik = o["iterations"][k]
        assert (int(g["K"][k]), int(g["C"][k])) == (ik["K"], ik["C"]), (case.name, k)
        if p["robust_kernel"]:
            assert int(g["iter_inliers"][k]) == ik["inliers"]
        print(f"    {case.name} inner iteration {k}: chi2 {float(g['chi2'][k]):.6g} vs {ik['chi2_fp64']:.6g}")
    # the statistics pass: Linearizer::update at the GPU's returned T on the finder's correspondences (FULL_H: all 34 sums)
    st = al._statistics
    Tinv0 = O.iso_inverse(case.guess)
    corr, _ = O.correspondences(ap, oref, ocur, o["ref_index"], o["cur_index"], Tinv0)
    os_ = O.align_statistics(ap, oref, ocur, g["T"])
    invT = O.iso_inverse(g["T"])
    ol = O.linearize(ap, oref, ocur, corr, invT)
    assert np.array_equal(os_["H"], ol["H"])
    assert st["inliers"] == ol["inliers"], (case.name, st["inliers"], ol["inliers"])
    assert _chi2_close(float(st["error"]), ol["chi2_fp64"]), (case.name, float(st["error"]), ol["chi2_fp64"])
    frac = _check_hb(f"{case.name} {storage} {over} statistics pass", st, ol, ra, ca, corr, invT, p, FUSED_CHAIN)
    # k_linearize_list on the oracle's list at the guess
    ol0 = O.linearize(ap, oref, ocur, corr, Tinv0)
    gl = al.linearize(corr, Tinv0)
    assert gl["inliers"] == ol0["inliers"] and _chi2_close(float(gl["chi2"]), ol0["chi2_fp64"]), case.name
    frac = max(frac, _check_hb(f"{case.name} {storage} {over} list", gl, ol0, ra, ca, corr, Tinv0, p, LIST_CHAIN))
    # part 3: the step
    step = float(np.abs(g["T"].astype(np.float64) - o["T"]).max())
    print(f"    {case.name} {storage} {over}: K {i0['K']} C {i0['C']} inliers {i0['inliers']} chi2 distance {chi2_d:.2e}; step distance {step:.2e} (bar {step_bar:.1e}; "
          f"oracle to float64 {step_note:.1e})")
    assert step <= step_bar, (case.name, step)
    return dict(K=i0["K"], C=i0["C"], inliers=i0["inliers"], chi2=chi2_d, frac=frac, step=step)


FAMILY_GUESSES = [(f, g) for f in A.SMALL_SIZES for g in A.GUESSES]


@pytest.mark.parametrize("storage", STORAGES)
def test_finder_equals_the_oracle_list(rig, oracle, storage):
    cases = [A.family_case(f, g) for f, g in FAMILY_GUESSES] + [A.mixed_case(480, 640), A.mixed_case(513, 640), A.mixed_case(480, 640, "moderate"),
                                                                 A.empty_case("rejected"), A.empty_case("none")]
    for case in cases:
        al, keep, (oref, ocur, ra, ca), ap, p = _pair(rig, oracle, case, storage)
        Tinv = oracle.iso_inverse(case.guess)
        ocorr, oK = oracle.correspondences(ap, oref, ocur, case.ref_index, case.cur_index, Tinv)
        gcorr, gK = al.computeCorrespondences(case.ref_index, case.cur_index, Tinv)
        assert gK == oK == int(case.candidates().sum()), case.name
        assert np.array_equal(gcorr, ocorr), (case.name, len(gcorr), len(ocorr))
        mcorr, _ = M.correspondences(ra, ca, case.ref_index, case.cur_index, Tinv, *_finder_args(p))
        assert np.array_equal(gcorr, mcorr), case.name


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("fam", list(A.SMALL_SIZES))
def test_fused_pass_teacher_forced(rig, oracle, storage, fam):
    """parts 2, 3 and 6: every family alone under the three guesses; robust kernel on and off, and inner_iterations = 2 (SAME_T = false)"""
    rows = []
    for guess in A.GUESSES:
        case = A.family_case(fam, guess)
        for over in ({}, {"robust_kernel": 0}, {"inner_iterations": 2}):
            if guess != "identity" and over and fam not in ("chi2_edge", "omega_range"):
                continue
            rows.append(_check_fused(rig, oracle, case, storage, **over))
    print(f"  {fam:13s} {storage}: candidates {sum(r['K'] for r in rows)}, correspondences {sum(r['C'] for r in rows)}, inliers {sum(r['inliers'] for r in rows)}, "
          f"worst chi2 distance {max(r['chi2'] for r in rows):.2e}, worst H/b error {max(r['frac'] for r in rows):.3f} of its bar, worst step {max(r['step'] for r in rows):.2e}")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("size", [(64, 32), (3, 683), (17, 65)] + list(A.LARGE_SIZES))
def test_fused_pass_mixed_sizes(rig, oracle, storage, size):
    """every family in one pair at the tiling's sizes: one tile, a second tile of one pixel, a partial tile, 150 tiles, and 160 / 161 tiles:
    the last record of reduce_partials' first trip and the first of its second"""
    case = A.mixed_case(*size)
    _check_fused(rig, oracle, case, storage)
    if size == (480, 640):
        _check_fused(rig, oracle, case, storage, robust_kernel=0)
        _check_fused(rig, oracle, A.mixed_case(480, 640, "moderate"), storage, inner_iterations=2)


def _quat_branch(oracle, T):
    """the branch of mat2quat that t2v takes on the matrix the solve step hands it (the guess through iso_inverse twice): -1 for trace > 0"""
    R = oracle.iso_inverse(oracle.iso_inverse(T))[:3, :3]
    t = np.float32(np.float32(R[0, 0] + R[1, 1]) + R[2, 2])
    if t > 0:
        return -1
    i = 1 if R[1, 1] > R[0, 0] else 0
    return 2 if R[2, 2] > (R[0, 0] if i == 0 else R[1, 1]) else i


@pytest.mark.parametrize("storage", STORAGES)
def test_mat2quat_branches_on_the_device(rig, oracle, storage):
    """dx = 0: the result is v2t(t2v(.)) of the guess through iso_inverse twice -- no summation order involved, the same source compiled with
    contraction off on both sides: the pose is the oracle's bit for bit"""
    taken = {0: 0, 1: 0, 2: 0}
    for name, G in A.big_guesses().items():
        for kind in ("none", "rejected") if name.endswith("150") else ("none",):
            case = A.make_case(f"empty_{kind}/{name}", 17, 65, G, {f"empty_{kind}": 200}, seed=5)
            al, keep, (oref, ocur, ra, ca), ap, p = _pair(rig, oracle, case, storage)
            br = _quat_branch(oracle, case.guess)
            assert br >= 0, name
            taken[br] += 1
            g = al.align()
            o = oracle.align(ap, oref, ocur)
            assert int(g["C"][0]) == 0 == o["iterations"][0]["C"] and float(g["chi2"][0]) == 0.0
            assert np.array_equal(g["T"].view(np.uint32), o["T"].view(np.uint32)), (name, kind, g["T"], o["T"])
    print(f"  trace <= 0 branches taken (largest diagonal entry 0, 1, 2): {taken}")
    assert min(taken.values()) >= 3, taken
    # the same guesses with a populated case: checks as in parts 2 and 3
    big = A.big_guesses()
    for name in ("x150", "y179", "z125", "skew180"):
        case = A.make_case(f"index_edges/{name}", 3, 683, big[name], {"index_edges": 300, "omega_range": 300}, seed=6)
        assert _quat_branch(oracle, case.guess) >= 0
        _check_fused(rig, oracle, case, storage)


RESULT_FIELDS = ("T", "error", "inliers", "iterations", "chi2", "iter_inliers", "iter_correspondences", "iter_candidates", "n_reference", "n_current")


@functools.lru_cache(maxsize=None)
def _compute_units():
    """Multiprocessor count of device 0 as torch reports it, asked in a process of its own: torch ships its own HIP runtime, and that runtime finds
    no device in a process where the library's runtime was initialised first (the other order, bench.py's, works)."""
    import subprocess
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-600:]
    return int(r.stdout.split()[-1])


@pytest.mark.parametrize("storage", STORAGES)
def test_both_kernel_shapes_give_the_same_records(rig, oracle, storage):
    """a launch of tiles x pairs <= CU count workgroups runs k_corr_linearize_lat, a larger one k_corr_linearize: single pairs against batches of
    the same pairs, in both orders and mixed with `empty` pairs, result records bitwise equal"""
    from g2o_frontend_amd import api
    cus = _compute_units()
    ctx = rig(storage)
    shapes = set()
    groups = []
    for rows, cols in A.LARGE_SIZES:
        groups.append([A.mixed_case(rows, cols), A.make_case("empty_none/large", rows, cols, "identity", {"empty_none": 400}, seed=9, tiles=[0, 5, 159]),
                       A.mixed_case(rows, cols)] + ([A.mixed_case(480, 640, "moderate")] if rows == 480 else []))
    groups.append([A.mixed_case(17, 65), A.empty_case("rejected"), A.family_case("chi2_edge"), A.empty_case("none"), A.family_case("chi2_edge", "small"),
                   A.empty_case("none", "moderate"), A.family_case("chi2_edge", "moderate"),
                   A.make_case("omega_range/17x65", 17, 65, "small", {"omega_range": 400, "cancel": 100}, seed=10)])
    for cases in groups:
        base = cases[0]
        al = A.gpu_aligner(ctx, base)
        clouds = [A.gpu_clouds(ctx, c) for c in cases]
        singles = []
        for c, (gr, gc) in zip(cases, clouds):
            assert (c.rows, c.cols) == (base.rows, base.cols) and c.params == base.params
            al.setReferenceCloud(gr); al.setCurrentCloud(gc); al.setInitialGuess(c.guess)
            singles.append(al.alignBatch([gr], [gc], [c.guess], raw=True)[0].copy())
            shapes.add("lat" if c.tiles * 1 <= cus else "throughput")
            r = al.align()                                             # pwn_hip_align and a batch of one: the same record
            assert np.array_equal(r["T"].T.reshape(-1).view(np.uint32), singles[-1]["T"].view(np.uint32))
        for sel in (list(range(len(cases))), list(range(len(cases)))[::-1]):
            res = al.alignBatch([clouds[i][0] for i in sel], [clouds[i][1] for i in sel], [cases[i].guess for i in sel], raw=True)
            shapes.add("lat" if base.tiles * len(sel) <= cus else "throughput")
            for k, i in enumerate(sel):
                for fld in RESULT_FIELDS:
                    a, b = np.asarray(res[k][fld]), np.asarray(singles[i][fld])
                    assert a.tobytes() == b.tobytes(), (base.rows, cases[i].name, fld, a, b)
        print(f"  {base.rows}x{base.cols}: {len(cases)} pairs, {base.tiles} tiles each, {cus} CUs")
    assert shapes == {"lat", "throughput"}, shapes
