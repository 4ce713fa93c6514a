"""Batch alignment with SE(3) priors on the device (pwn_hip_align_batch_priors) against the single call (pwn_hip_align_with_priors_ex), pair by
pair and bit for bit -- the header's contract: a batch of n equals n single calls, through every sub-batch and stream plan, with the cloud's
own index image or a projection, so a difference is a bug, not a tolerance.  The single call is ONE PAIR OF THE SAME BATCH CALL (the loop the
host once drove behind it is gone): these comparisons hold the call to itself across batch sizes, sub-batch and stream plans -- they find a
pair that reads another pair's list or state, not a loop that is wrong for every pair alike.  What the loop computes is held to the CPU oracle
in tests/test_gpu_prior_steps.py.  Also: a call without priors against the existing calls, record packing, the convergence setting, the
settle-fault repeat, the refusals and the mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import early_stop as E
from conftest import case_params, make_depth_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = tuple(range(9))
KINDS = ("identity", "odometry", "far")
INFO = (np.diag([4e5, 4e5, 4e5, 2e6, 2e6, 2e6]) + 1e4).astype(np.float32)      # tests/test_priors.py
THRESHOLD = 50.0


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cm(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).reshape(4, 4).T.reshape(-1))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def prior_lists(seeds):
    """per pair a list of (kind, mean, referenceTransform, information): none, one relative, one absolute, absolute + relative (tracker2's
    order), three -- means a few centimetres off the pair's pose, so that each prior moves the solution"""
    from g2o_frontend_amd import synth
    reft = synth.v2t(np.array([0.02, 0.01, -0.01, 0.0, 0.01, 0.0]))
    out = []
    for i, s in enumerate(seeds):
        P = synth.pair_pose(s)
        rel = lambda d: (0, (P @ synth.v2t(np.array(d))).astype(np.float32), np.eye(4, dtype=np.float32), INFO)
        ab = lambda d: (1, (reft @ P @ synth.v2t(np.array(d))).astype(np.float32), reft.astype(np.float32), (INFO * 0.5).astype(np.float32))
        out.append([[], [rel([0.03, -0.02, 0.01, 0.01, -0.01, 0.005])], [ab([-0.02, 0.03, 0.02, -0.01, 0.0, 0.01])],
                    [ab([0.02, 0.01, -0.03, 0.0, 0.01, -0.01]), rel([-0.01, -0.02, 0.02, 0.005, 0.01, 0.0])],
                    [rel([0.03, 0.0, 0.0, 0.0, 0.0, 0.01]), ab([0.0, 0.02, 0.0, 0.01, 0.0, 0.0]), rel([0.0, 0.0, -0.02, 0.0, -0.01, 0.0])]][i % 5])
    return out


def prior_array(lists):
    """(pwn_hip_pair_priors, what keeps its arrays alive)"""
    import prior_cases as pc
    from g2o_frontend_amd import _lib
    n = len(lists)
    first = np.zeros(n + 1, np.int32); first[1:] = np.cumsum([len(q) for q in lists])
    arr = (_lib.Prior * max(int(first[n]), 1))()
    for j, prior in enumerate([p for q in lists for p in q]):
        arr[j] = pc.prior_struct(prior)
    return _lib.PairPriors(first.ctypes.data_as(C.POINTER(C.c_int)), C.cast(arr, C.POINTER(_lib.Prior))), (first, arr)


def stat_words(st):
    """[n, 47] float32 of an AlignStatistics array in the closure record's order: omega, mean, both ratios, error, inliers, computed"""
    out = np.zeros((len(st), 47), np.float32)
    for i, q in enumerate(st):
        out[i, :36] = np.frombuffer(q.omega, np.float32); out[i, 36:42] = np.frombuffer(q.mean, np.float32)
        out[i, 42] = np.float32(q.translational_eigen_ratio); out[i, 43] = np.float32(q.rotational_eigen_ratio)
        out[i, 44] = np.float32(q.error); out[i, 45] = np.float32(q.inliers); out[i, 46] = 1.0
    return out


def packed(res, ids, score=None, stats=None):
    """the record of include/pwn_hip.h packed on the host from a pair's pwn_hip_align_result (structured array element), its score
    (image_non_zeros, image_outliers, image_inliers, image_reprojection_distance) and its statistics words: 64, 72 or 128 floats"""
    n = 128 if stats is not None else 72 if score is not None else 64
    w = np.zeros(n, np.float32)
    it = int(res["iterations"]); m = min(it, 10)
    w[:16] = res["T"]; w[16] = res["error"]; w[17] = res["inliers"]; w[18] = it; w[19] = ids
    w[20:20 + m] = res["chi2"][:m]; w[30:30 + m] = res["iter_inliers"][:m]; w[40:40 + m] = res["iter_correspondences"][:m]
    w[50:50 + m] = res["iter_candidates"][:m]
    w[60] = res["n_reference"]; w[61] = res["n_current"]; w[62] = m
    if score is not None:
        w[64:68] = score
    if stats is not None:
        w[72:119] = stats
    return w


class Rig:
    def __init__(self, storage, seeds=SEEDS, max_batch=16):
        from g2o_frontend_amd import api
        from test_gpu_parity import gpu_objects
        self.rows, self.cols, self.K, _, _ = case_params("small")
        self.ctx = api.Context(0, self.rows, self.cols, max_batch, omega_storage=storage)
        _, self.converter, self.aligner = gpu_objects(self.ctx, "small")
        self.refs, self.curs = [], []
        for s in seeds:
            ref, cur, _, _, _ = make_depth_pair("small", s)
            r, c = api.Cloud(self.ctx, self.rows * self.cols), api.Cloud(self.ctx, self.rows * self.cols)
            self.converter.compute(r, ref, images=False); self.converter.compute(c, cur, images=False)
            self.refs.append(r); self.curs.append(c)
        self.guesses = [E.guess_for(s, KINDS[i % 3]) for i, s in enumerate(seeds)]
        self.lists = prior_lists(seeds)
        self._single = {}

    def args(self, idx):
        n = len(idx)
        return (n, (C.c_void_p * n)(*[self.refs[i].h for i in idx]), (C.c_void_p * n)(*[self.curs[i].h for i in idx]),
                np.stack([_cm(self.guesses[i]) for i in idx]))

    def params(self, outer=None):
        p = self.aligner.params()
        if outer is not None:
            p.outer_iterations = outer
        return p

    def batch(self, idx, record_floats=0, lists=None, ids=None, first=0, outer=None, results=True, priors=True):
        """pwn_hip_align_batch_priors -> dict(res, sc, st, stw [n, 47], rec)"""
        from g2o_frontend_amd import api
        from g2o_frontend_amd._lib import AlignStatistics, MatchResult
        ctx, p = self.ctx, self.params(outer)
        n, refs, curs, g = self.args(idx)
        pp, keep = prior_array([self.lists[i] for i in idx] if lists is None else lists)
        res = (api.AlignResult * n)() if results else None; sc = (MatchResult * n)(); st = (AlignStatistics * n)()
        rec = np.full((n, record_floats), -7.0, np.float32) if record_floats else None
        ctx.check(ctx._L.pwn_hip_align_batch_priors(ctx.h, C.byref(p), n, refs, curs, _vp(g), C.byref(pp) if priors else None, THRESHOLD, _vp(ids), first,
                                                    res, sc, st, _vp(rec), record_floats))
        out = dict(sc=np.frombuffer(sc, np.int32).reshape(n, 4).copy(), st=st, stw=stat_words(st), rec=rec)
        if results:
            r = np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=n).copy(); r["total_time_ms"] = 0
            out["res"] = r
        return out

    def single_call(self, i, outer=None):
        """pwn_hip_align_with_priors_ex of pair i (no priors: pwn_hip_align_batch_ex for one pair) and pwn_hip_match_score behind it; cached"""
        if (i, outer) not in self._single:
            self._single[(i, outer)] = self.single_call_of(self.refs[i], self.curs[i], i, outer)
        return self._single[(i, outer)]

    def single_call_of(self, ref, cur, i, outer=None, images=False):
        """the same call for the clouds ref, cur with pair i's guess and prior list; images: pwn_hip_align_images behind the score"""
        from g2o_frontend_amd import api
        from g2o_frontend_amd._lib import AlignStatistics, MatchResult, Prior
        import prior_cases as pc
        ctx, p = self.ctx, self.params(outer)
        C.memmove(p.initial_guess, _cm(self.guesses[i]).ctypes.data, 64)
        arr = (Prior * max(len(self.lists[i]), 1))()
        for j, prior in enumerate(self.lists[i]):
            arr[j] = pc.prior_struct(prior)
        res = api.AlignResult(); st = (AlignStatistics * 1)(); sc = MatchResult()
        ctx.check(ctx._L.pwn_hip_align_with_priors_ex(ctx.h, C.byref(p), ref.h, cur.h, len(self.lists[i]), arr, C.byref(res), st))
        ctx.check(ctx._L.pwn_hip_match_score(ctx.h, THRESHOLD, C.byref(sc)))
        r = np.frombuffer(bytes(res), dtype=api.ALIGN_RESULT_DTYPE, count=1).copy(); r["total_time_ms"] = 0
        out = dict(res=r[0], sc=np.frombuffer(bytes(sc), np.int32).copy(), scf=np.frombuffer(bytes(sc), np.float32).copy(), stw=stat_words(st)[0],
                   H=bytes(st[0].H), b=bytes(st[0].b))
        if images:
            ri = np.empty((p.rows, p.cols), np.int32); ci = np.empty((p.rows, p.cols), np.int32)
            rd = np.empty((p.rows, p.cols), np.float32); cd = np.empty((p.rows, p.cols), np.float32)
            ctx.check(ctx._L.pwn_hip_align_images(ctx.h, _vp(ri), _vp(rd), _vp(ci), _vp(cd)))
            out["images"] = (ri, rd.view(np.uint32), ci, cd.view(np.uint32))
        return out

    def close(self):
        self.ctx.close()


def same_pair(got, k, want, what):
    """pair k of a batch call against a single call: T, chi2, inliers, ncorr, ncand, iterations (the whole result), score, statistics"""
    assert got["res"][k].tobytes() == want["res"].tobytes(), (what, "result", got["res"][k]["T"], want["res"]["T"], got["res"][k]["chi2"][:10], want["res"]["chi2"][:10])
    assert np.array_equal(got["sc"][k], want["sc"]), (what, "score")
    assert np.array_equal(_bits(got["stw"][k]), _bits(want["stw"])), (what, "statistics")
    assert bytes(got["st"][k].H) == want["H"] and bytes(got["st"][k].b) == want["b"], (what, "H, b of the statistics")


@pytest.fixture(scope="module", params=["sym6", "exact9"])
def rig(request):
    r = Rig(request.param)
    yield r
    r.close()


@pytest.mark.parametrize("n", [1, 5, 9])
def test_every_pair_equals_one_pair_of_the_same_call(rig, n):
    """a batch of n equals n single calls, each of them one pair of the batch call itself (no independent loop is left to compare with: the
    oracle holds the loop in tests/test_gpu_prior_steps.py): sub-batches of 4 (9 runs as 4 + 4 + 1) on 1 and on 4 streams, and the default plan"""
    idx = list(range(n))
    want = [rig.single_call(i) for i in idx]
    for sub, streams in ((4, 1), (4, 4), (64, 4)):
        rig.ctx.set_subbatch(64, sub); rig.ctx.set_concurrency(streams)
        try:
            got = rig.batch(idx)
        finally:
            rig.ctx.set_subbatch(64, 64); rig.ctx.set_concurrency(4)
        for k, i in enumerate(idx):
            same_pair(got, k, want[i], (n, sub, streams, i))
    if n == 9:      # a pair with priors ends elsewhere than the same pair without, a pair without ends where it did (how much a prior matters: the oracle test)
        free = rig.batch(idx, priors=False)
        for k in idx:
            moved = np.abs(free["res"][k]["T"] - got["res"][k]["T"]).max()
            assert (moved > 0) == bool(rig.lists[k]), (k, moved)


def test_prior_terms_run_once_per_inner_iteration_of_a_sub_batch_with_priors(rig):
    ctx = rig.ctx
    ms, launches = C.c_float(0), C.c_int(0)
    outer = rig.params().outer_iterations * rig.params().inner_iterations
    ctx._L.pwn_hip_set_profiling(ctx.h, 1)
    try:
        ctx.set_subbatch(64, 4)
        rig.batch(list(range(9)))                   # 4 + 4 + 1: pair 0 and pair 5 carry none, every sub-batch holds a prior
        ctx.check(ctx._L.pwn_hip_last_stage_ms(ctx.h, b"prior_terms", C.byref(ms), C.byref(launches)))
        assert launches.value == 3 * outer and ms.value > 0
        rig.batch([0, 5, 1])                        # sub-batch size 4 holds all three: one launch per iteration
        ctx.check(ctx._L.pwn_hip_last_stage_ms(ctx.h, b"prior_terms", C.byref(ms), C.byref(launches)))
        assert launches.value == outer
        rig.batch([0, 5])                           # no prior anywhere: the kernel is not launched
        ctx.check(ctx._L.pwn_hip_last_stage_ms(ctx.h, b"prior_terms", C.byref(ms), C.byref(launches)))
        assert launches.value == 0
    finally:
        ctx.set_subbatch(64, 64); ctx._L.pwn_hip_set_profiling(ctx.h, 0)


def test_a_call_without_priors_equals_the_existing_calls(rig):
    """pair_priors == NULL and an all-empty list: every record word of the three record calls, results, scores and statistics of pwn_hip_align_batch_ex"""
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import AlignStatistics, MatchResult
    ctx, L, p = rig.ctx, rig.ctx._L, rig.params()
    idx = list(range(9)); n, refs, curs, g = rig.args(idx)
    ids = np.arange(40, 40 + n, dtype=np.int32)[::-1].copy()
    r64 = np.full((n, 64), -7.0, np.float32); r72 = np.full((n, 72), -7.0, np.float32); r128 = np.full((n, 128), -7.0, np.float32)
    ctx.check(L.pwn_hip_align_batch_records(ctx.h, C.byref(p), n, refs, curs, _vp(g), _vp(ids), 0, None, _vp(r64)))
    ctx.check(L.pwn_hip_match_batch_records(ctx.h, C.byref(p), n, refs, curs, _vp(g), THRESHOLD, _vp(ids), 0, None, None, _vp(r72)))
    ctx.check(L.pwn_hip_closure_batch_records(ctx.h, C.byref(p), n, refs, curs, _vp(g), THRESHOLD, _vp(ids), 0, None, None, None, _vp(r128)))
    res = (api.AlignResult * n)(); sc = (MatchResult * n)(); st = (AlignStatistics * n)()
    ctx.check(L.pwn_hip_align_batch_ex(ctx.h, C.byref(p), n, refs, curs, _vp(g), res, THRESHOLD, sc, st))
    r = np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=n).copy(); r["total_time_ms"] = 0
    empty = [[] for _ in idx]
    for kw in (dict(priors=False), dict(lists=empty)):
        for want, floats in ((r64, 64), (r72, 72), (r128, 128)):
            got = rig.batch(idx, record_floats=floats, ids=ids, **kw)
            assert np.array_equal(_bits(got["rec"]), _bits(want)), (kw.keys(), floats)
        got = rig.batch(idx, **kw)
        assert got["res"].tobytes() == r.tobytes() and np.array_equal(got["sc"], np.frombuffer(sc, np.int32).reshape(n, 4))
        assert np.array_equal(_bits(got["stw"]), _bits(stat_words(st)))
    # and inside a call WITH priors, the pairs that carry none
    mixed = rig.batch(idx)
    for k in idx:
        if not rig.lists[k]:
            assert mixed["res"][k].tobytes() == r[k].tobytes() and np.array_equal(_bits(mixed["stw"][k]), _bits(stat_words(st)[k]))


def test_batch_of_nine_equals_nine_calls_of_one(rig):
    idx = list(range(9))
    nine = rig.batch(idx, record_floats=128, first=5)
    for k in idx:
        one = rig.batch([k], record_floats=128, first=5 + k)
        assert one["res"][0].tobytes() == nine["res"][k].tobytes() and np.array_equal(one["sc"][0], nine["sc"][k])
        assert np.array_equal(_bits(one["rec"][0]), _bits(nine["rec"][k])), k


def test_records_in_all_three_forms_equal_host_packing_of_the_host_results(rig):
    """the host results: what the single calls returned to the host"""
    idx = list(range(9))
    ids = np.arange(100, 109, dtype=np.int32)
    want = [rig.single_call(i) for i in idx]
    for floats in (64, 72, 128):
        got = rig.batch(idx, record_floats=floats, ids=ids, results=(floats != 72))
        for k in idx:
            w = want[k]
            score = None if floats == 64 else np.array([w["sc"][0], w["sc"][1], w["sc"][2], w["scf"][3]], np.float32)
            ref = packed(w["res"], ids[k], score, w["stw"] if floats == 128 else None)
            assert np.array_equal(_bits(got["rec"][k]), _bits(ref)), (floats, k, np.where(_bits(got["rec"][k]) != _bits(ref))[0][:8])
    # the closure record's statistics words are the single call's statistics
    assert all(np.array_equal(_bits(got["rec"][k, 72:119]), _bits(want[k]["stw"])) for k in idx)


def _same_single(a, b, what):
    assert a["res"].tobytes() == b["res"].tobytes(), (what, "result")
    assert a["sc"].tobytes() == b["sc"].tobytes() and a["scf"].tobytes() == b["scf"].tobytes(), (what, "score")
    assert np.array_equal(_bits(a["stw"]), _bits(b["stw"])) and a["H"] == b["H"] and a["b"] == b["b"], (what, "statistics")


@pytest.mark.parametrize("i", [1, 3])
def test_single_call_with_the_index_shortcut_equals_the_projection(rig, i):
    """pair 1 carries a relative prior, pair 3 an absolute and a relative one.  The rig's clouds carry their converter's index image, so the single
    call takes it in place of projecting the current cloud (pwn_hip_debug_set_index_shortcut); result, statistics, the score behind it and the
    finder's four images are those of the call that projects"""
    ctx = rig.ctx
    assert [len(rig.lists[k]) for k in (1, 3)] == [1, 2] and [q[0] for q in rig.lists[3]] == [1, 0]
    try:
        ctx.check(ctx._L.pwn_hip_debug_set_index_shortcut(ctx.h, 1))
        on = rig.single_call_of(rig.refs[i], rig.curs[i], i, images=True)
        ctx.check(ctx._L.pwn_hip_debug_set_index_shortcut(ctx.h, 0))
        off = rig.single_call_of(rig.refs[i], rig.curs[i], i, images=True)
    finally:
        ctx.check(ctx._L.pwn_hip_debug_set_index_shortcut(ctx.h, 1))
    _same_single(on, off, i)
    for a, b, name in zip(on["images"], off["images"], ("reference index", "reference depth", "current index", "current depth")):
        assert np.array_equal(a, b), (i, name)
    assert (on["images"][2] >= 0).sum() > 1000       # the images are not empty


def test_single_call_with_priors_leaves_stage_times_and_takes_the_index_shortcut(rig):
    """with profiling on a single call with priors has stage times like every alignment call, and they say whether the current cloud was
    projected: not with the shortcut (the comparison above is not one of a call with itself), once without"""
    ctx = rig.ctx
    ms, launches = C.c_float(0), C.c_int(0)
    p = rig.params()
    ctx._L.pwn_hip_set_profiling(ctx.h, 1)
    try:
        for shortcut, projections in ((1, 0), (0, 1)):
            ctx.check(ctx._L.pwn_hip_debug_set_index_shortcut(ctx.h, shortcut))
            rig.single_call_of(rig.refs[3], rig.curs[3], 3)
            ctx.check(ctx._L.pwn_hip_last_stage_ms(ctx.h, b"project_cur", C.byref(ms), C.byref(launches)))
            assert launches.value == projections, shortcut
            ctx.check(ctx._L.pwn_hip_last_stage_ms(ctx.h, b"prior_terms", C.byref(ms), C.byref(launches)))
            assert launches.value == p.outer_iterations * p.inner_iterations and ms.value > 0
    finally:
        ctx.check(ctx._L.pwn_hip_debug_set_index_shortcut(ctx.h, 1)); ctx._L.pwn_hip_set_profiling(ctx.h, 0)


def test_single_call_on_uploaded_clouds_equals_one_pair_of_the_batch(rig):
    """uploaded clouds have no index image of their own: the current cloud is projected; single call and n = 1 of the batch call, the same bits"""
    from g2o_frontend_amd import api
    i = 3
    up = []
    for src in (rig.refs[i], rig.curs[i]):
        a = src.arrays()
        c = api.Cloud(rig.ctx, rig.rows * rig.cols)
        c.upload(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])
        up.append(c)
    one = rig.single_call_of(up[0], up[1], i)
    refs, curs = rig.refs[i], rig.curs[i]
    rig.refs[i], rig.curs[i] = up
    try:
        got = rig.batch([i])
    finally:
        rig.refs[i], rig.curs[i] = refs, curs
    same_pair(got, 0, one, "uploaded")


@pytest.mark.parametrize("kind", [0, 1])
def test_one_pair_against_the_oracle(oracle, kind):
    """n = 1 of the new call through the Python mirror against the CPU oracle's align() with the same prior, which is shown to matter"""
    from g2o_frontend_amd import api, synth
    from test_gpu_parity import gpu_objects, _check_alignment
    rows, cols, K, conv, alig = case_params("small")
    ref, cur, _, _, _ = make_depth_pair("small", 1)
    cp = oracle.converter_params(K=K, **conv)
    cr, _, _ = oracle.convert(cp, ref); cc, _, _ = oracle.convert(cp, cur)
    ctx = api.Context(0, rows, cols, 2)
    try:
        _, converter, aligner = gpu_objects(ctx, "small")
        gref, gcur = api.Cloud(ctx, rows * cols), api.Cloud(ctx, rows * cols)
        converter.compute(gref, ref); converter.compute(gcur, cur)
        mean = synth.v2t(np.array([0.06, -0.03, -0.02, 0.01, -0.015, 0.01])).astype(np.float32)
        reft = synth.v2t(np.array([0.02, 0.01, -0.01, 0.0, 0.01, 0.0])).astype(np.float32)
        ap = oracle.aligner_params(rows, cols, K=K, accumulate_fp64=1, **alig)
        oracle.clear_priors()
        free = oracle.align(ap, cr, cc)
        if kind == 0:
            oracle.add_prior(0, mean, INFO); prior = (0, mean, np.eye(4, dtype=np.float32), INFO)
        else:
            oracle.add_prior(1, mean, INFO, reference_transform=reft); prior = (1, mean, reft, INFO)
        o = oracle.align(ap, cr, cc)
        g = aligner.alignBatch([gref], [gcur], priors=[[prior]])[0]
        assert np.abs(o["T"] - free["T"]).max() > 1e-3            # the prior matters in this set-up
        _check_alignment(o, g)
        steps = ctx.last_align_steps(0, 1)[0]
        assert steps["iterations"] == alig["outer_iterations"] and np.all(steps["step_translation"] > 0)
    finally:
        oracle.clear_priors()
        ctx.close()


def test_convergence_setting_is_honoured(rig):
    """pairs that stop at different iterations return the bits of the call with that outer_iterations; the step traces are filled"""
    idx = list(range(9))
    rig.ctx.set_convergence(*E.LOOSE)
    try:
        got = rig.batch(idx, record_floats=128)
        steps = rig.ctx.last_align_steps(0, 9)
    finally:
        rig.ctx.clear_convergence()
    inner = rig.params().inner_iterations
    stops = [s["iterations"] for s in steps]
    print("outer iterations per pair:", stops)
    assert len(set(stops)) > 1 and min(stops) < rig.params().outer_iterations
    for k in idx:
        assert got["res"][k]["iterations"] == stops[k] * inner
        assert steps[k]["converged"] == (E.stop_iteration(steps[k]["step_translation"], steps[k]["step_rotation"], E.LOOSE, 10 ** 6) <= stops[k])
        assert E.stop_iteration(steps[k]["step_translation"], steps[k]["step_rotation"], E.LOOSE, stops[k]) == stops[k]
        want = rig.batch([k], record_floats=128, first=k, outer=stops[k])
        assert want["res"][0].tobytes() == got["res"][k].tobytes(), k
        assert np.array_equal(_bits(want["rec"][0]), _bits(got["rec"][k])) and np.array_equal(want["sc"][0], got["sc"][k]), k
        same_pair(got, k, rig.single_call(k, outer=stops[k]), ("stopped", k))


def test_settle_fault_repeat_returns_the_same_bits(rig):
    ctx = rig.ctx
    idx = [1, 2, 3, 4, 5]
    want = rig.batch(idx, record_floats=128)
    before, after = C.c_int(0), C.c_int(0)
    ctx.check(ctx._L.pwn_hip_debug_projection_fallbacks(ctx.h, C.byref(before)))
    ctx.check(ctx._L.pwn_hip_debug_set_settle_guard(ctx.h, 0))
    try:
        got = rig.batch(idx, record_floats=128)
    finally:
        ctx.check(ctx._L.pwn_hip_debug_set_settle_guard(ctx.h, -1))
    ctx.check(ctx._L.pwn_hip_debug_projection_fallbacks(ctx.h, C.byref(after)))
    assert after.value == before.value + 1
    assert got["res"].tobytes() == want["res"].tobytes() and np.array_equal(_bits(got["rec"]), _bits(want["rec"]))
    assert np.array_equal(got["sc"], want["sc"]) and np.array_equal(_bits(got["stw"]), _bits(want["stw"]))


def test_refusals_touch_nothing(rig):
    from g2o_frontend_amd import api, _lib
    ctx, L, p = rig.ctx, rig.ctx._L, rig.params()
    idx = [1, 2, 3]; n, refs, curs, g = rig.args(idx)
    lists = [rig.lists[i] for i in idx]
    pp, keep = prior_array(lists)
    first, arr = keep

    def call(pp, rec, floats):
        res = (api.AlignResult * n)()
        C.memset(res, 0x5A, C.sizeof(res))
        before = bytes(res)
        rc = L.pwn_hip_align_batch_priors(ctx.h, C.byref(p), n, refs, curs, _vp(g), C.byref(pp), THRESHOLD, None, 0, res, None, None, _vp(rec), floats)
        assert (bytes(res) == before) == (rc != 0)
        return rc

    rec = np.full((n, 128), -7.0, np.float32)
    assert call(pp, None, 0) == 0
    for bad_first in ([1, 1, 2, 3], [0, 2, 1, 3], [0, 1, -1, 3]):
        f = np.array(bad_first, np.int32)
        assert call(_lib.PairPriors(f.ctypes.data_as(C.POINTER(C.c_int)), pp.priors), rec, 128) == 1
    assert call(_lib.PairPriors(None, pp.priors), rec, 128) == 1
    assert call(_lib.PairPriors(pp.first, None), rec, 128) == 1                       # null array with first[n] > 0
    kind = arr[1].kind
    for bad_kind in (2, -1):
        arr[1].kind = bad_kind
        assert call(pp, rec, 128) == 1
    arr[1].kind = kind
    for floats in (1, 63, 65, 127, 256, -64):
        assert call(pp, rec, floats) == 1
    assert call(pp, None, 64) == 1 and call(pp, rec, 0) == 1
    assert (rec == -7.0).all()
    assert b"prior" in L.pwn_hip_last_error_string(ctx.h) or b"record" in L.pwn_hip_last_error_string(ctx.h)
    assert call(pp, rec, 128) == 0 and not (rec == -7.0).any()


def test_python_mirror_equals_the_c_abi(rig):
    idx = list(range(9))
    lists = [rig.lists[i] for i in idx]
    refs = [rig.refs[i] for i in idx]; curs = [rig.curs[i] for i in idx]; guesses = [rig.guesses[i] for i in idx]
    want = rig.batch(idx, record_floats=64, first=3)
    raw = rig.aligner.alignBatch(refs, curs, initialGuesses=guesses, raw=True, priors=lists).copy()
    raw["total_time_ms"] = 0
    assert raw.tobytes() == want["res"].tobytes()
    rec = np.full((9, 64), -7.0, np.float32)
    res = rig.aligner.alignBatchRecords(refs, curs, rec, first_pair_id=3, initialGuesses=guesses, priors=lists).copy()
    res["total_time_ms"] = 0
    assert res.tobytes() == want["res"].tobytes() and np.array_equal(_bits(rec), _bits(want["rec"]))
    # without `priors` the mirror makes the call it made before: the bits of a call whose pairs carry none
    free = rig.batch(idx, priors=False)
    plain = rig.aligner.alignBatch(refs, curs, initialGuesses=guesses, raw=True).copy(); plain["total_time_ms"] = 0
    assert plain.tobytes() == free["res"].tobytes()


def test_cpp_mirror_reproduces_the_python_mirrors_records(tmp_path):
    """tools/pwn_hip_batch_priors_check: Aligner::alignBatchRecords / alignBatch of the C++ mirror with the same frames, guesses and prior lists"""
    import struct
    from g2o_frontend_amd import api, build
    from test_gpu_parity import gpu_objects
    import prior_cases as pc
    build.build_tools()
    rows, cols, K, _, _ = case_params("small")
    seeds = (0, 1, 2, 3, 4)
    n = len(seeds)
    ctx = api.Context(0, rows, cols, 16)
    try:
        _, converter, aligner = gpu_objects(ctx, "small")
        raw = [make_depth_pair("small", s)[3:5] for s in seeds]
        refs = [api.Cloud(ctx, rows * cols) for _ in range(n)]; curs = [api.Cloud(ctx, rows * cols) for _ in range(n)]
        converter.computeBatch(refs + curs, [r for r, _ in raw] + [c for _, c in raw], raw_scale=0.001)
        guesses = [E.guess_for(s, KINDS[i % 3]) for i, s in enumerate(seeds)]
        lists = prior_lists(seeds)
        rec = np.full((n, api.RECORD_FLOATS), -7.0, np.float32)
        aligner.alignBatchRecords(refs, curs, rec, first_pair_id=40, initialGuesses=guesses, priors=lists)
        outer, inner = aligner.params().outer_iterations, aligner.params().inner_iterations
    finally:
        ctx.close()
    first = np.zeros(n + 1, np.int32); first[1:] = np.cumsum([len(q) for q in lists])
    path = os.path.join(str(tmp_path), "batch_priors.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<6i4f", n, rows, cols, outer, inner, 40, *[float(np.float32(k)) for k in K]))
        for r, c in raw:
            f.write(np.ascontiguousarray(r, np.uint16).tobytes()); f.write(np.ascontiguousarray(c, np.uint16).tobytes())
        for T in guesses:
            f.write(_cm(T).tobytes())
        f.write(first.tobytes())
        for q in lists:
            for prior in q:
                f.write(bytes(pc.prior_struct(prior)))
        f.write(rec.tobytes())
    exe = os.path.join(ROOT, "tools", "pwn_hip_batch_priors_check")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 differences" in r.stdout and f"{int(first[n])} priors" in r.stdout
    # the tool finds a changed word
    bad = rec.copy(); bad[1, 3] = np.nextafter(bad[1, 3], np.float32(np.inf))
    with open(path, "r+b") as f:
        f.seek(-rec.nbytes, 2); f.write(bad.tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "record 1 differs from word 3" in r.stderr
