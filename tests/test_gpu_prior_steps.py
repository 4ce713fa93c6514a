"""The device loop with SE(3) priors (k_prior_terms and k_solve_update_priors inside align_batch_impl, behind pwn_hip_align_with_priors_ex and
pwn_hip_align_batch_priors) against the CPU oracle's Aligner::align with the same priors, on the injected clouds of tests/prior_steps.py, in
both Omega_p storages and both cloud forms (uploaded: tests/test_gpu_align_clouds.py; the converter's: tests/test_gpu_converter_form.py).
Since the loop the host once drove is gone, every other test of the calls with priors compares the device loop with itself or runs ten
free-running iterations against loose bars; this file is the independent hold.  The bars come from tests/test_prior_steps_cpu.py, which
measures the oracle against a float64 model and shows that each wrong loop named below lies at least 100 bars away.

  A  single call (Aligner.addRelativePrior / addAbsolutePrior, align), one outer iteration from the case's guess, every case x every list x
     inner_iterations 1 and 2: images bit for bit, counters equal, chi2 within CHI2_RTOL, |T - T_oracle| <= PRIOR_STEP_BAR, and the statistics
     pass's H, b, error, inliers against oracle.linearize (no prior in it) at the returned T.  Catches: priors dropped, terms of a later inner
     iteration missing or taken at a stale invT, a refused prior's record added, terms left in the statistics' H.
  B  one call with outer_iterations 2 (3 on one case): counters of every iteration, the pose within the bar for that many iterations, the
     step traces.  Catches: terms taken at the pose of the previous outer iteration.
  C  Aligner.alignBatch(..., priors=[...]) of nine pairs with different lists, two orders, three sub-batch / stream plans, and the three
     record lengths: every pair against the oracle's step for that pair with that pair's list.  Catches: another pair's list, a sub-batch
     without priors beside one with.
"""
import ctypes as C

import numpy as np
import pytest

import align_clouds as A
import prior_steps as PS
import test_gpu_align_clouds as GA
import test_gpu_batch_priors as BP
import test_gpu_converter_form as GC
from test_prior_steps_cpu import PRIOR_OUTER_BAR, STEP_BARS

pytestmark = pytest.mark.gpu

STORAGES = GA.STORAGES
MAKERS = {"uploaded": GA.uploaded, "converter": GC.maker(*PS.CONVERTER_FORM)}
PLANS = ((4, 1), (4, 4), (64, 4))             # (pairs per sub-batch, streams); the last is the default plan
THRESHOLD = 50.0
_ctx = {}
_made = {}
_worst = {}


@pytest.fixture(scope="module")
def rig():
    from g2o_frontend_amd import api

    def get(storage):
        if storage not in _ctx:
            _ctx[storage] = api.Context(device=0, max_rows=64, max_cols=683, max_batch=16, omega_storage=storage)
        return _ctx[storage]
    yield get
    _made.clear()
    for c in _ctx.values():
        for k in [k for k in GC._clouds if k[0] == id(c)]:      # the converter-form maker keeps its clouds per context
            del GC._clouds[k]
        c.close()
    _ctx.clear()


def _note(part, value, bar, where):
    if value / bar > _worst.get(part, (0.0, None))[0]:
        _worst[part] = (value / bar, where)


def _say(part):
    w = _worst.get(part)
    if w:
        print(f"  part {part}: worst pose distance {w[0]:.3f} of its bar at {w[1]}")


def _clouds(ctx, oracle, case, storage, form):
    """((reference, current) GPU clouds, (reference, current) oracle clouds, (reference, current) arrays), made once: nothing writes them"""
    key = (id(ctx), case.name, storage, form)
    if key not in _made:
        _made[key] = MAKERS[form](ctx, case, storage, oracle)
    return _made[key]


def _aligner(rig, oracle, case, storage, form, plist, **over):
    ctx = rig(storage)
    (gref, gcur), oc, (ra, ca) = _clouds(ctx, oracle, case, storage, form)
    assert gcur.omega_storage() == storage
    al = A.gpu_aligner(ctx, case, **over)
    al.setReferenceCloud(gref); al.setCurrentCloud(gcur)          # setting a cloud clears the priors: they are added behind it
    for kind, mean, reft, info in plist:
        if kind == 0:
            al.addRelativePrior(mean, info)
        else:
            al.addAbsolutePrior(reft, mean, info)
    return al, oc, (ra, ca)


def _same_counters(g, o, robust, where):
    assert g["iterations"] == len(o["iterations"]), where
    for k, it in enumerate(o["iterations"]):
        assert (int(g["K"][k]), int(g["C"][k])) == (it["K"], it["C"]), (where, k)
        if k == 0 or robust:       # without the robust kernel the inliers of a later iteration are an fp32 decision at each side's own iterate
            assert int(g["iter_inliers"][k]) == it["inliers"], (where, k)


# ------------------------------------------------------------------------------------------------------------ A. the single call
def _check_single(rig, oracle, case, storage, form, name, inner, over):
    O = oracle
    plist = PS.prior_list(case, name)
    where = (case.name, storage, form, name, inner, over)
    al, oc, (ra, ca) = _aligner(rig, O, case, storage, form, plist, inner_iterations=inner, **over)
    p = dict(case.params, inner_iterations=inner, **over)
    g = al.align(images=True, statistics=True)
    o = PS.oracle_step(O, case, oc, plist, inner, **over)
    f = al.correspondenceFinder()
    assert np.array_equal(f.referenceIndexImage(), o["ref_index"]) and np.array_equal(f.currentIndexImage(), o["cur_index"]), where
    assert np.array_equal(f.referenceDepthImage().view(np.uint32), o["ref_depth"].view(np.uint32)), where
    assert np.array_equal(f.currentDepthImage().view(np.uint32), o["cur_depth"].view(np.uint32)), where
    _same_counters(g, o, p["robust_kernel"], where)
    i0 = o["iterations"][0]
    assert i0["C"] >= 100
    assert GA._chi2_close(float(g["chi2"][0]), i0["chi2_fp64"]), (where, float(g["chi2"][0]), i0["chi2_fp64"])
    step = PS.distance(g["T"], o["T"])
    print(f"    {where}: C {i0['C']}, pose distance {step:.2e} ({step / STEP_BARS[form]:.3f} of its bar)")
    _note("A", step, STEP_BARS[form], where)
    assert step <= STEP_BARS[form], (where, step)
    # the statistics pass: Linearizer::update at the returned T on the finder's correspondences, the prior terms not in it (aligner.cpp:165-170)
    st = al._statistics
    ap = A.oracle_params(O, case, inner_iterations=inner, **over)
    corr, _ = O.correspondences(ap, oc[0], oc[1], o["ref_index"], o["cur_index"], O.iso_inverse(case.guess))
    invT = O.iso_inverse(g["T"])
    ol = O.linearize(ap, oc[0], oc[1], corr, invT)
    assert st["inliers"] == ol["inliers"], (where, st["inliers"], ol["inliers"])
    assert GA._chi2_close(float(st["error"]), ol["chi2_fp64"]), (where, float(st["error"]), ol["chi2_fp64"])
    GA._check_hb(f"{where} statistics pass", st, ol, ra, ca, corr, invT, p, GA.FUSED_CHAIN)
    return g, st


def _bits_of(g, st):
    return (g["T"].tobytes(), g["chi2"].tobytes(), g["iter_inliers"].tobytes(), g["C"].tobytes(), g["K"].tobytes(),
            st["H"].tobytes(), st["b"].tobytes(), np.asarray(st["omega"]).tobytes(), np.asarray(st["mean"]).tobytes(), st["error"], st["inliers"])


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("form", PS.FORMS)
@pytest.mark.parametrize("ci", range(PS.N_CASES))
def test_single_call_against_the_oracle(rig, oracle, storage, form, ci):
    case = PS.all_cases()[ci]
    free = {}
    for c, name, inner, over in PS.part_a():
        if c is case:
            g, st = _check_single(rig, oracle, case, storage, form, name, inner, over)
            if name == "none":
                free[(inner, tuple(over.items()))] = _bits_of(g, st)
    # lists that hold refused priors only: the bits of the call without priors
    r0, r1 = PS.prior_list(case, "refused_front")[0], PS.prior_list(case, "refused_middle")[1]
    assert PS.is_refused(r0) and PS.is_refused(r1) and (r0[0], r1[0]) == (0, 1)
    for plist in ([r0], [r1, r0]):
        for inner in (1, 2):
            al, _, _ = _aligner(rig, oracle, case, storage, form, plist, inner_iterations=inner)
            g = al.align(statistics=True)
            assert _bits_of(g, al._statistics) == free[(inner, ())], (case.name, len(plist), inner)
    _say("A")


# ------------------------------------------------------------------------------------------------------------ B. outer iterations in one call
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("form", PS.FORMS)
def test_outer_iterations_in_one_call_against_the_oracle(rig, oracle, storage, form):
    ran = set()
    for case, name, inner, outer in PS.part_b():
        plist = PS.prior_list(case, name)
        if not PS.outer_fit(oracle, case, form, plist, inner, outer)[0]:      # judged from the reference side (tests/test_prior_steps_cpu.py)
            continue
        where = (case.name, storage, form, name, inner, outer)
        al, oc, _ = _aligner(rig, oracle, case, storage, form, plist, inner_iterations=inner, outer_iterations=outer)
        g = al.align()
        o = PS.oracle_step(oracle, case, oc, plist, inner, outer, images=False)
        assert g["iterations"] == inner * outer
        _same_counters(g, o, True, where)
        d = PS.distance(g["T"], o["T"])
        print(f"    {where}: pose distance {d:.2e} ({d / PRIOR_OUTER_BAR[outer]:.3f} of its bar)")
        _note("B", d, PRIOR_OUTER_BAR[outer], where)
        assert d <= PRIOR_OUTER_BAR[outer], (where, d)
        steps = rig(storage).last_align_steps(0, 1)[0]
        assert steps["iterations"] == outer and len(steps["step_translation"]) == outer == len(steps["step_rotation"]), where
        assert np.all(steps["step_translation"] > 0) and np.all(steps["step_rotation"] > 0), where
        ran.add((case.name, outer))
    assert len({c for c, _ in ran}) >= 3 and {n for _, n in ran} == set(PS.OUTERS), ran
    _say("B")


# ------------------------------------------------------------------------------------------------------------ C. the batch
def _batch_rig(rig, oracle, storage, form):
    ctx = rig(storage)
    cases = PS.batch_cases()
    made = [_clouds(ctx, oracle, c, storage, form) for c in cases]
    return ctx, cases, [m[0] for m in made], [m[1] for m in made], PS.batch_lists(cases)


def _oracle_steps(oracle, cases, oclouds, lists, inner):
    return [PS.oracle_step(oracle, c, oc, q, inner, images=False) for c, oc, q in zip(cases, oclouds, lists)]


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("form", PS.FORMS)
@pytest.mark.parametrize("inner", [1, 2])
def test_batch_against_the_oracle_pair_by_pair(rig, oracle, storage, form, inner):
    """every pair of the batch call against the oracle's step of THAT pair with THAT pair's list -- not against n = 1 of the same call"""
    ctx, cases, clouds, oclouds, lists = _batch_rig(rig, oracle, storage, form)
    want = _oracle_steps(oracle, cases, oclouds, lists, inner)
    al = A.gpu_aligner(ctx, cases[0], inner_iterations=inner)
    try:
        for order in PS.ORDERS:
            for sub, streams in PLANS:
                ctx.set_subbatch(64, sub); ctx.set_concurrency(streams)
                res = al.alignBatch([clouds[i][0] for i in order], [clouds[i][1] for i in order], [cases[i].guess for i in order],
                                    priors=[lists[i] for i in order])
                for k, i in enumerate(order):
                    where = (cases[i].name, storage, form, inner, order, sub, streams, k)
                    _same_counters(res[k], want[i], True, where)
                    assert GA._chi2_close(float(res[k]["chi2"][0]), want[i]["iterations"][0]["chi2_fp64"]), where
                    d = PS.distance(res[k]["T"], want[i]["T"])
                    _note("C", d, STEP_BARS[form], where)
                    assert d <= STEP_BARS[form], (where, d)
    finally:
        ctx.set_subbatch(64, 64); ctx.set_concurrency(4)
    _say("C")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("form", PS.FORMS)
def test_batch_records_against_the_oracle(rig, oracle, storage, form):
    """pwn_hip_align_batch_priors with records of 64, 72 and 128 floats, sub-batches of four on four streams: the pose, the counters, the
    iteration count and the pair id of every record against the oracle's step for that pair"""
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import AlignStatistics, MatchResult
    inner = 2
    ctx, cases, clouds, oclouds, lists = _batch_rig(rig, oracle, storage, form)
    want = _oracle_steps(oracle, cases, oclouds, lists, inner)
    order = PS.ORDERS[0]; n = len(order)
    p = A.gpu_aligner(ctx, cases[0], inner_iterations=inner).params()
    refs = (C.c_void_p * n)(*[clouds[i][0].h for i in order]); curs = (C.c_void_p * n)(*[clouds[i][1].h for i in order])
    g = np.stack([BP._cm(cases[i].guess) for i in order])
    pp, keep = BP.prior_array([lists[i] for i in order])
    ids = np.arange(300, 300 + n, dtype=np.int32)
    ctx.set_subbatch(64, 4)
    try:
        for floats in (64, 72, 128):
            rec = np.full((n, floats), -7.0, np.float32)
            res = (api.AlignResult * n)(); sc = (MatchResult * n)(); st = (AlignStatistics * n)()
            ctx.check(ctx._L.pwn_hip_align_batch_priors(ctx.h, C.byref(p), n, refs, curs, BP._vp(g), C.byref(pp), THRESHOLD, BP._vp(ids), 0, res, sc, st,
                                                        BP._vp(rec), floats))
            for k, i in enumerate(order):
                where = (cases[i].name, storage, form, floats, k)
                w, o = rec[k], want[i]
                d = PS.distance(w[:16].reshape(4, 4).T, o["T"])
                _note("C records", d, STEP_BARS[form], where)
                assert d <= STEP_BARS[form], (where, d)
                assert (int(w[18]), int(w[19]), int(w[62])) == (inner, int(ids[k]), inner), where
                for j, it in enumerate(o["iterations"]):
                    assert (int(w[30 + j]), int(w[40 + j]), int(w[50 + j])) == (it["inliers"], it["C"], it["K"]), (where, j)
                assert GA._chi2_close(float(w[20]), o["iterations"][0]["chi2_fp64"]), where
    finally:
        ctx.set_subbatch(64, 64)
    _say("C records")
