"""The alignment loop with SE(3) priors on the injected clouds of tests/prior_steps.py, from the reference side only: the oracle's fp32 loop
(oracle.add_prior, then oracle.align) against the float64 model_step over everything tests/test_gpu_prior_steps.py runs, and the conditions
under which that GPU test can decide anything -- each a condition of this test: where one fails, other inputs are chosen, the condition stays.

  * the measured distances stay below the constants here, from which the GPU bars are derived (never from a GPU run):
        PRIOR_STEP_BAR = max(5e-6, 4 x ORACLE_PRIOR_STEP_DISTANCE), the same for the converter's form and per outer-iteration count;
    5e-6 and the factor 4 are tests/test_gpu_align_clouds.py::STEP_BAR's: the other summation order of the device sums;
  * every wrong loop of prior_steps.VARIANTS moves the model's result by at least DECISIVE = 100 bars wherever it applies;
  * a refused prior is really refused: the oracle returns the same bits with it in the list as with it removed;
  * the priors matter: the result with them lies at least 100 bars from the result without;
  * a case enters the one-call outer_iterations > 1 part only where prior_steps.outer_fit holds; at least three cases remain.
"""
import numpy as np

import align_clouds as A
import numpy_reference_model as M
import prior_steps as PS

# worst |oracle's fp32 step with priors - model_step| (max over the 4 x 4) after one outer iteration, inner_iterations 1 and 2, as
# test_oracle_step_with_priors_against_the_model measures and asserts it
ORACLE_PRIOR_STEP_DISTANCE = 1e-6             # measured: 7.7e-7 (prior/cancel/d/moderate, absolute+relative, inner 2)
CONVERTER_FORM_PRIOR_STEP_DISTANCE = 7e-7     # measured: 5.5e-7 (prior/single3x683/moderate, three, inner 2)
# the same after outer_iterations = 2 and 3 in one call, on the fit cases (test_outer_iterations_in_one_call)
ORACLE_PRIOR_OUTER_DISTANCE = {2: 7e-7, 3: 2e-7}      # measured: 5.3e-7 (converter form, prior/edges/b/moderate, absolute, inner 1); 1.3e-7 (prior/cancel/b/small)
PRIOR_STEP_BAR = max(5e-6, 4 * ORACLE_PRIOR_STEP_DISTANCE)
CONVERTER_FORM_PRIOR_STEP_BAR = max(5e-6, 4 * CONVERTER_FORM_PRIOR_STEP_DISTANCE)
PRIOR_OUTER_BAR = {n: max(5e-6, 4 * d) for n, d in ORACLE_PRIOR_OUTER_DISTANCE.items()}
STEP_BARS = {"uploaded": PRIOR_STEP_BAR, "converter": CONVERTER_FORM_PRIOR_STEP_BAR}
STEP_DISTANCES = {"uploaded": ORACLE_PRIOR_STEP_DISTANCE, "converter": CONVERTER_FORM_PRIOR_STEP_DISTANCE}
DECISIVE = 100
FUSED_CHAIN = A.CHAIN


class _Extremes:
    """worst (largest) and least values with where they occurred"""
    def __init__(self):
        self.hi, self.lo = {}, {}

    def add(self, key, value, where):
        if key not in self.hi or value > self.hi[key][0]:
            self.hi[key] = (value, where)
        if key not in self.lo or value < self.lo[key][0]:
            self.lo[key] = (value, where)

    def report(self, title):
        print(title)
        for k in sorted(self.hi):
            print(f"  {k:34s} worst {self.hi[k][0]:.2e} at {self.hi[k][1]}\n  {'':34s} least {self.lo[k][0]:.2e} at {self.lo[k][1]}")


_clouds = {}


def _setup(O, case, form):
    key = (case.name, form)
    if key not in _clouds:
        arrs = PS.arrays(case, form)
        _clouds[key] = (arrs, PS.oracle_clouds(O, arrs))
    return _clouds[key]


def test_model_inputs_are_the_oracles(oracle):
    """the fp32 inverse the model hands its finder is the oracle's, the oracle projects the index images the generator intended, and the model's
    finder gives the oracle's list on them"""
    for case in PS.all_cases():
        assert np.array_equal(oracle.iso_inverse(case.guess).view(np.uint32), PS.inverse_f32(case.guess).view(np.uint32)), case.name
        for form in PS.FORMS:
            arrs, oc = _setup(oracle, case, form)
            o = PS.oracle_step(oracle, case, oc, [])
            assert np.array_equal(o["ref_index"], case.ref_index) and np.array_equal(o["cur_index"], case.cur_index), case.name
            ap = A.oracle_params(oracle, case)
            ocorr, oK = oracle.correspondences(ap, oc[0], oc[1], case.ref_index, case.cur_index, oracle.iso_inverse(case.guess))
            m = PS.model_step(case, arrs, (case.ref_index, case.cur_index), [], 1)
            assert np.array_equal(m["corr"], ocorr) and m["iterations"][0]["K"] == oK == int(case.candidates().sum()), case.name
            assert len(ocorr) >= 100, (case.name, len(ocorr))


def test_lists_are_what_they_claim():
    for case in PS.all_cases():
        kinds = {name: [(q[0], PS.is_refused(q)) for q in PS.prior_list(case, name)] for name in PS.LISTS}
        assert kinds == {"none": [], "relative": [(0, False)], "absolute": [(1, False)], "absolute+relative": [(1, False), (0, False)],
                         "three": [(0, False), (1, False), (0, False)], "refused_middle": [(0, False), (1, True), (1, False)],
                         "refused_front": [(0, True), (1, False), (0, False)]}, case.name
        for name in PS.LISTS:
            for kind, mean, reft, info in PS.prior_list(case, name):
                assert (kind == 1) == (not np.array_equal(reft, np.eye(4, dtype=np.float32)))          # an absolute prior's reference transform is no identity
                if not PS.is_refused((kind, mean, reft, info)):      # the mean lies centimetres and a fraction of a degree off the guess
                    e = M._t2v(PS.inv64(case.guess) @ PS.inv64(reft) @ mean.astype(np.float64))
                    assert 0.005 < np.abs(e[:3]).max() < 0.05 and 0.001 < np.abs(e[3:]).max() < 0.01, (case.name, name, e)
    # the batch: every list occurs, and two pairs carry none
    assert sorted(set(PS.BATCH_LISTS)) == list(range(len(PS.LISTS))) and PS.BATCH_LISTS.count(0) == 2
    assert len({(c.rows, c.cols) for c in PS.batch_cases()}) == 1 and all(c.params == A.PARAMS for c in PS.batch_cases())
    for order in PS.ORDERS:
        assert sorted(order) == list(range(len(PS.batch_cases())))
    first, last = PS.ORDERS
    assert PS.BATCH_LISTS[first[0]] == 0 and PS.BATCH_LISTS[first[8]] == 0            # opens a sub-batch of four; a sub-batch of its own
    assert PS.BATCH_LISTS[last[3]] == 0 and PS.BATCH_LISTS[last[7]] == 0              # closes a sub-batch of four, twice


def test_oracle_step_with_priors_against_the_model(oracle):
    """one outer iteration from the case's guess, every (case, list, inner, robust) of the single-call part in both cloud forms: the distance,
    that the priors matter, that the refused prior is refused, and that the wrong loops "none", "stale_inner", "first_inner_only" and
    "in_statistics" are decisive"""
    O = oracle
    dist, var = _Extremes(), _Extremes()
    for form in PS.FORMS:
        bar = STEP_BARS[form]
        for case, name, inner, over in PS.part_a():
            arrs, oc = _setup(O, case, form)
            plist = PS.prior_list(case, name)
            where = (case.name, name, f"inner {inner}", over)
            o = PS.oracle_step(O, case, oc, plist, inner, **over)
            idx = (o["ref_index"], o["cur_index"])
            m = PS.model_step(case, arrs, idx, plist, inner, **over)
            assert len(o["iterations"]) == inner
            i0, m0 = o["iterations"][0], m["iterations"][0]
            assert (i0["K"], i0["C"], i0["inliers"]) == (m0["K"], m0["C"], m0["inliers"]), where
            dist.add(form, PS.distance(o["T"], m["T"]), where)
            valid = PS.without_refused(plist)
            if len(valid) != len(plist):
                kept = PS.oracle_step(O, case, oc, valid, inner, **over)
                assert np.array_equal(kept["T"].view(np.uint32), o["T"].view(np.uint32)), where
                assert [i["chi2"] for i in kept["iterations"]] == [i["chi2"] for i in o["iterations"]], where
            if not valid:
                continue
            wrong = lambda v: PS.model_step(case, arrs, idx, plist, inner, variant=v, **over)
            var.add(f"{form} none / bar", PS.distance(wrong("none")["T"], m["T"]) / bar, where)
            free = PS.oracle_step(O, case, oc, [], inner, **over)
            var.add(f"{form} oracle without priors / bar", PS.distance(free["T"], o["T"]) / bar, where)
            if inner > 1:
                for v in ("stale_inner", "first_inner_only"):
                    var.add(f"{form} {v} / bar", PS.distance(wrong(v)["T"], m["T"]) / bar, where)
            # the statistics H with the terms left in, against the bar tests/test_gpu_align_clouds.py::_check_hb holds that H to
            w = wrong("in_statistics")
            assert np.array_equal(w["T"], m["T"])
            barH, _ = A.hb_bar(m["stat_Habs"], np.zeros(6), m["stat_H"], np.zeros(6), FUSED_CHAIN)
            dH = np.abs(w["stat_H"] - m["stat_H"])
            var.add(f"{form} in_statistics / H bar", float((dH / np.maximum(barH, 1e-300)).max()), where)
            var.add(f"{form} in_statistics / bar", float(dH.max()) / bar, where)
    dist.report("oracle-to-model distance after one outer iteration with priors:")
    var.report("how far a wrong loop moves the model, in bars:")
    for form in PS.FORMS:
        assert dist.hi[form][0] <= STEP_DISTANCES[form], (form, dist.hi[form])
    for k, (v, where) in var.lo.items():
        assert v >= DECISIVE, (k, v, where)


def test_the_neighbours_list_is_decisive(oracle):
    """every adjacent pair of both batch orders: the model with the next pair's list ends at least 100 bars from the model with its own"""
    O = oracle
    cases, lists = PS.batch_cases(), PS.batch_lists()
    var = _Extremes()
    for form in PS.FORMS:
        for order in PS.ORDERS:
            for a, b in zip(order[:-1], order[1:]):
                arrs, _ = _setup(O, cases[a], form)
                idx = (cases[a].ref_index, cases[a].cur_index)
                for inner in (1, 2):
                    own = PS.model_step(cases[a], arrs, idx, lists[a], inner)
                    nb = PS.model_step(cases[a], arrs, idx, lists[a], inner, variant="neighbour", neighbour=lists[b])
                    var.add(f"{form} neighbour / bar", PS.distance(own["T"], nb["T"]) / STEP_BARS[form], (cases[a].name, cases[b].name, f"inner {inner}"))
    var.report("how far the next pair's list moves the model, in bars:")
    for k, (v, where) in var.lo.items():
        assert v >= DECISIVE, (k, v, where)


def test_outer_iterations_in_one_call(oracle):
    """outer_iterations = 2 (3 on one case) in one call: which candidates are fit, the oracle-to-model distance on the fit ones, and that taking
    the terms at the previous outer iteration's invT is decisive"""
    O = oracle
    dist, var = _Extremes(), _Extremes()
    fit_cases = {form: set() for form in PS.FORMS}
    unfit = []
    for form in PS.FORMS:
        for case, name, inner, outer in PS.part_b():
            plist = PS.prior_list(case, name)
            where = (form, case.name, name, f"inner {inner}", f"outer {outer}")
            fit, o, m = PS.outer_fit(O, case, form, plist, inner, outer)
            if not fit:
                unfit.append(where)
                continue
            fit_cases[form].add(case.name)
            dist.add(f"outer {outer}", PS.distance(o["T"], m["T"]), where)
            arrs, _ = _setup(O, case, form)
            stale = PS.model_step(case, arrs, (case.ref_index, case.cur_index), plist, inner, outer, variant="stale_outer")
            var.add(f"stale_outer, outer {outer} / bar", PS.distance(stale["T"], m["T"]) / PRIOR_OUTER_BAR[outer], where)
    print(f"fit cases: { {f: len(v) for f, v in fit_cases.items()} } of {len(PS.all_cases())}; unfit candidates: {unfit}")
    dist.report("oracle-to-model distance after outer_iterations in one call:")
    var.report("how far stale terms move the model, in bars:")
    for form in PS.FORMS:
        assert len(fit_cases[form]) >= 3, (form, fit_cases[form])
    assert set(dist.hi) == {f"outer {n}" for n in PS.OUTERS}
    for n in PS.OUTERS:
        assert dist.hi[f"outer {n}"][0] <= ORACLE_PRIOR_OUTER_DISTANCE[n], dist.hi[f"outer {n}"]
    for k, (v, where) in var.lo.items():
        assert v >= DECISIVE, (k, v, where)
