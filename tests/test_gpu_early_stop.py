""""Stop when converged" on the device (include/pwn_hip.h: pwn_hip_ctx_set_convergence, pwn_hip_last_align_steps).

What must hold:
  * off by default, and a context that had the setting on and switched it off computes the bits of a fresh one;
  * the recorded step norms (feature off): entry 0 against the CPU oracle's first step from the same iterate (5e-6, docs/parity.md "The step"),
    later entries against the library's own poses of consecutive iteration counts (STEP_FROM_POSES_BAR below);
  * THE CONTRACT: with k* taken from the disabled run's own traces by the model of tests/early_stop.py, every output of a pair -- result, both
    record forms, matchClouds score, statistics, step traces, and for the pair of slot 0 the finder's images and pwn_hip_match_score -- equals bit
    for bit that of the call with outer_iterations = k*; total_time_ms is exempt;
  * `<=` at equality on both sides, min_iterations, inner_iterations = 2, the one-submission steps, the two-pass projection, priors, the mirrors.

Shapes: six 120 x 160 pairs (k_corr_linearize_lat; with and without the index-image shortcut), 32 pairs in sub-batches of 8 on two streams (slots
and tags reused from sub-batch to sub-batch; 10 workgroups per pair x 8 pairs still fit the device, so this is the latency shape too -- the
throughput shape k_corr_linearize is what the VGA batch runs: 150 workgroups per pair x 3), n = 1 and n = 3 (k_solve_update writes the host's
copy of the state itself), and one 17 x 65 pair of injected clouds (a partial single tile, every projection executed).
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import early_stop as E
from conftest import case_params, make_depth_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
# |recorded s[i] - norm of t2v(inv(T_{i+1}) T_i)| for i >= 1, T_k = the library's pose after k iterations.  Between the two stands the
# renormalisation T = v2t(t2v(.)) of every outer iteration and the fp32 rounding of both poses' entries (2^-24 of entries up to 1 in the rotation,
# of a few centimetres in the translation).  Measured on MI355X over the six pairs and iterations 1..9 (docs/parity.md, "Step norms"): 5.4e-8 in the
# translation, 1.6e-8 in the rotation; entry 0 lies 7.5e-9 from the oracle's.  The bar is four times the measured worst.
STEP_FROM_POSES_BAR_T = 4 * 5.4e-8
STEP_FROM_POSES_BAR_R = 4 * 1.6e-8


def _cm(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).reshape(4, 4).T.reshape(-1))


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Rig:
    """a context, the reference-style objects of a configuration, the clouds of its pairs; every distinct call is made once"""

    def __init__(self, ctx, aligner, refs, curs, converter=None):
        self.ctx, self.aligner, self.refs, self.curs, self.converter = ctx, aligner, refs, curs, converter
        self.cache = {}

    def handles(self, idx):
        n = len(idx)
        return (C.c_void_p * n)(*[self.refs[i].h for i in idx]), (C.c_void_p * n)(*[self.curs[i].h for i in idx])

    def setup(self, outer, inner, setting):
        if setting is None:
            self.ctx.clear_convergence()
        else:
            self.ctx.set_convergence(*setting)
        self.aligner.setOuterIterations(outer); self.aligner.setInnerIterations(inner)
        return self.aligner.params()

    def run_min(self, idx, guesses, outer, setting=None, inner=1, key=None):
        """pwn_hip_align_batch: results (total_time_ms zeroed) and step traces"""
        from g2o_frontend_amd import api
        k = ("min", tuple(idx), key, outer, inner, setting)
        if key is not None and k in self.cache:
            return self.cache[k]
        p = self.setup(outer, inner, setting)
        n = len(idx)
        refs, curs = self.handles(idx)
        g = np.stack([_cm(T) for T in guesses])
        res = (api.AlignResult * n)()
        self.ctx.check(self.ctx._L.pwn_hip_align_batch(self.ctx.h, C.byref(p), n, refs, curs, _vp(g), res))
        r = np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=n).copy(); r["total_time_ms"] = 0
        out = dict(res=r, steps=self.aligner.lastSteps(0, n))
        self.ctx.clear_convergence()
        if key is not None:
            self.cache[k] = out
        return out

    def run_all(self, idx, guesses, outer, setting=None, inner=1, key=None):
        """every output the contract names: pwn_hip_align_batch_ex (results, scores, statistics), the step traces, the finder's images and
        pwn_hip_match_score of slot 0 where the call left them, pwn_hip_match_batch_records without results (72-word records; the step traces then
        come from the device on request) and pwn_hip_align_batch_records (64-word records)"""
        from g2o_frontend_amd import api
        from g2o_frontend_amd._lib import AlignStatistics, MatchResult
        k = ("all", tuple(idx), key, outer, inner, setting)
        if key is not None and k in self.cache:
            return self.cache[k]
        ctx, L = self.ctx, self.ctx._L
        p = self.setup(outer, inner, setting)
        n = len(idx)
        refs, curs = self.handles(idx)
        g = np.stack([_cm(T) for T in guesses])
        res = (api.AlignResult * n)(); sc = (MatchResult * n)(); st = (AlignStatistics * n)()
        ctx.check(L.pwn_hip_align_batch_ex(ctx.h, C.byref(p), n, refs, curs, _vp(g), res, 50.0, sc, st))
        r = np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=n).copy(); r["total_time_ms"] = 0
        out = dict(res=r, scores=np.frombuffer(sc, np.uint8).reshape(n, -1).copy(), stats=np.frombuffer(st, np.uint8).reshape(n, -1).copy(),
                   steps=self.aligner.lastSteps(0, n))
        ri = np.empty((p.rows, p.cols), np.int32); ci = np.empty((p.rows, p.cols), np.int32)
        rd = np.empty((p.rows, p.cols), np.float32); cd = np.empty((p.rows, p.cols), np.float32)
        out["images"] = None
        if L.pwn_hip_align_images(ctx.h, _vp(ri), _vp(rd), _vp(ci), _vp(cd)) == 0:       # a batch that skipped its current projections leaves none
            ms = MatchResult()
            ctx.check(L.pwn_hip_match_score(ctx.h, 50.0, C.byref(ms)))
            out["images"] = (ri, rd.view(np.uint32), ci, cd.view(np.uint32), np.frombuffer(ms, np.uint8).copy())
        rec72 = np.full((n, api.MATCH_RECORD_FLOATS), -7.0, np.float32)
        ctx.check(L.pwn_hip_match_batch_records(ctx.h, C.byref(p), n, refs, curs, _vp(g), 50.0, None, 7, None, None, _vp(rec72)))
        out["steps_after_records_only"] = self.aligner.lastSteps(0, n)
        rec64 = np.full((n, api.RECORD_FLOATS), -7.0, np.float32)
        ctx.check(L.pwn_hip_align_batch_records(ctx.h, C.byref(p), n, refs, curs, _vp(g), None, 7, None, _vp(rec64)))
        out["rec72"], out["rec64"] = rec72.view(np.uint32), rec64.view(np.uint32)
        ctx.clear_convergence()
        if key is not None:
            self.cache[k] = out
        return out


def _same_steps(a, b):
    return (a["iterations"] == b["iterations"] and a["step_translation"].tobytes() == b["step_translation"].tobytes()
            and a["step_rotation"].tobytes() == b["step_rotation"].tobytes())


def _stops(steps, setting, outer):
    return [E.stop_iteration(s["step_translation"], s["step_rotation"], setting, outer) for s in steps]


def check_contract(rig, idx, guesses, setting, outer, inner=1, key=None, slot0=0):
    """the enabled run against one disabled run per distinct k*; returns (k* per pair, enabled run)"""
    off = rig.run_all(idx, guesses, outer, None, inner, key)
    assert all(s["iterations"] == outer and not s["converged"] for s in off["steps"])
    ks = _stops(off["steps"], setting, outer)
    on = rig.run_all(idx, guesses, outer, setting, inner, key)
    want = {k: (off if k == outer else rig.run_all(idx, guesses, k, None, inner, key)) for k in sorted(set(ks))}
    for i, k in enumerate(ks):
        w, tag = want[k], (i, k)
        assert on["res"][i].tobytes() == w["res"][i].tobytes(), tag
        assert on["res"]["iterations"][i] == k * inner and (on["res"]["chi2"][i][k * inner:] == 0).all(), tag
        for f in ("scores", "stats", "rec72", "rec64"):
            assert on[f][i].tobytes() == w[f][i].tobytes(), (tag, f)
        assert on["rec64"][i].view(np.float32)[18] == k * inner and on["rec72"][i].view(np.float32)[62] == min(k * inner, 10), tag
        assert _same_steps(on["steps"][i], w["steps"][i]) and _same_steps(on["steps_after_records_only"][i], w["steps"][i]), tag
        s = off["steps"][i]
        stopped = any(j + 1 >= setting[2] and s["step_translation"][j] <= np.float32(setting[0]) and s["step_rotation"][j] <= np.float32(setting[1])
                      for j in range(outer))
        assert on["steps"][i]["converged"] == stopped and on["steps_after_records_only"][i]["converged"] == stopped, tag
        # what the disabled run recorded up to k* is what the enabled run recorded
        assert on["steps"][i]["step_translation"].tobytes() == s["step_translation"][:k].tobytes(), tag
    w = want[ks[slot0]]
    assert (on["images"] is None) == (w["images"] is None)
    if on["images"] is not None:
        for a, b in zip(on["images"], w["images"]):
            assert np.array_equal(a, b), ("slot 0", ks[slot0])
    return ks, on


# ------------------------------------------------------------------------------------------------------------ the rigs
@pytest.fixture(scope="module")
def small():
    """the six 120 x 160 pairs, exact9 clouds (bit for bit the oracle's), a context for up to 32 pairs"""
    from g2o_frontend_amd import api
    from test_gpu_parity import gpu_objects
    rows, cols, _, _, _ = case_params("small")
    ctx = api.Context(0, rows, cols, 32, omega_storage="exact9")
    _, converter, aligner = gpu_objects(ctx, "small")
    refs, curs = [], []
    for ref, cur in E.frames("small", E.SEEDS):
        r, c = api.Cloud(ctx, rows * cols), api.Cloud(ctx, rows * cols)
        converter.compute(r, ref, images=False); converter.compute(c, cur, images=False)
        refs.append(r); curs.append(c)
    yield Rig(ctx, aligner, refs, curs, converter)
    ctx.close()


ALL6 = list(range(6))


def _shortcut(ctx, on):
    ctx.check(ctx._L.pwn_hip_debug_set_index_shortcut(ctx.h, 1 if on else 0))


# ------------------------------------------------------------------------------------------------------------ 1. default off
def test_off_by_default_round_trip_and_refusals(small):
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import Convergence
    ctx = api.Context(0, 120, 160, 2)
    try:
        assert ctx.convergence() is None
        ctx.set_convergence(1e-3, 1e-4, 3)
        assert ctx.convergence() == dict(translation=float(np.float32(1e-3)), rotation=float(np.float32(1e-4)), min_iterations=3)
        for bad in ((-1e-3, 1e-4, 0), (1e-3, -1e-4, 0), (float("nan"), 1e-4, 0), (1e-3, float("nan"), 0), (float("inf"), 1e-4, 0), (1e-3, float("inf"), 0),
                    (1e-3, 1e-4, -1)):
            with pytest.raises(api.PwnHipError) as e:
                ctx.set_convergence(*bad)
            assert e.value.code == INVALID
            assert ctx.convergence()["min_iterations"] == 3          # a refused setting changes nothing
        ctx.set_convergence(0.0, 0.0)                                # zero is a setting: only a zero step stops
        assert ctx.convergence() == dict(translation=0.0, rotation=0.0, min_iterations=0)
        s = Convergence(0, 5.0, 5.0, 5)                              # enabled == 0: off, whatever the other fields say
        ctx.check(ctx._L.pwn_hip_ctx_set_convergence(ctx.h, C.byref(s)))
        assert ctx.convergence() is None
        ctx.set_convergence(1e-3, 1e-4); ctx.clear_convergence()
        assert ctx.convergence() is None
        # the step readout of a context that has not aligned, and ranges outside the last call
        with pytest.raises(api.PwnHipError):
            ctx.last_align_steps(0, 1)
    finally:
        ctx.close()
    small.run_min([0, 1], [np.eye(4)] * 2, 2)
    assert len(small.ctx.last_align_steps(1, 1)) == 1
    with pytest.raises(api.PwnHipError):
        small.ctx.last_align_steps(1, 2)                             # pair 2 of a call of two


def test_enable_run_disable_gives_the_bits_of_a_fresh_context():
    from g2o_frontend_amd import api
    from test_gpu_parity import gpu_objects
    rows, cols, _, _, _ = case_params("small")
    pairs = E.frames("small", E.SEEDS[:2])
    guesses = [E.guess_for(0, "identity"), E.guess_for(1, "odometry")]

    def rig():
        ctx = api.Context(0, rows, cols, 4)
        _, converter, aligner = gpu_objects(ctx, "small")
        refs = [api.Cloud(ctx, rows * cols) for _ in pairs]; curs = [api.Cloud(ctx, rows * cols) for _ in pairs]
        for (ref, cur), r, c in zip(pairs, refs, curs):
            converter.compute(r, ref, images=False); converter.compute(c, cur, images=False)
        return Rig(ctx, aligner, refs, curs)

    fresh = rig()
    a = fresh.run_all([0, 1], guesses, E.OUTER)
    fresh.ctx.close()
    used = rig()
    on = used.run_all([0, 1], guesses, E.OUTER, E.LOOSE)
    assert (on["res"]["iterations"] < E.OUTER).all()                  # it did stop them
    used.ctx.clear_convergence()
    b = used.run_all([0, 1], guesses, E.OUTER)
    used.ctx.close()
    for f in ("res", "scores", "stats", "rec72", "rec64"):
        assert a[f].tobytes() == b[f].tobytes(), f
    assert all(_same_steps(x, y) for x, y in zip(a["steps"], b["steps"]))


# ------------------------------------------------------------------------------------------------------------ 2. the recorded norms
def test_first_step_norm_against_the_oracle(small, oracle):
    """same clouds (exact9: the oracle's bits), same iterate (the guess): the project's bar for one step"""
    guesses = E.batch_guesses()
    off = small.run_all(ALL6, guesses, E.OUTER, None, key="mixed")
    worst = 0.0
    for i, s in enumerate(E.SEEDS):
        ap, oref, ocur = E.oracle_pair(oracle, "small", s, guess=guesses[i], outer_iterations=1)
        st, sr, _ = E.oracle_step_trace(oracle, ap, oref, ocur)
        dt = abs(float(off["steps"][i]["step_translation"][0]) - float(st[0])); dr = abs(float(off["steps"][i]["step_rotation"][0]) - float(sr[0]))
        print(f"pair {i}: s_t {off['steps'][i]['step_translation'][0]:.9e} oracle {st[0]:.9e} |d| {dt:.2e}   s_r {off['steps'][i]['step_rotation'][0]:.9e} oracle {sr[0]:.9e} |d| {dr:.2e}")
        worst = max(worst, dt, dr)
    print("worst difference of entry 0 from the oracle:", worst)
    assert worst <= 5e-6


def _motion_norms(Ta, Tb):
    """norms of the translation and of the quaternion vector of inv(Tb) Ta, float64 (the antisymmetric part: no cancellation at small angles)"""
    A = np.asarray(Ta, np.float64).reshape(4, 4).T; B = np.asarray(Tb, np.float64).reshape(4, 4).T      # column-major in the results
    Bi = np.eye(4); Bi[:3, :3] = B[:3, :3].T; Bi[:3, 3] = -B[:3, :3].T @ B[:3, 3]
    M = Bi @ A
    R = M[:3, :3]
    qw = 0.5 * np.sqrt(max(0.0, 1.0 + np.trace(R)))
    q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4.0 * qw)
    return float(np.linalg.norm(M[:3, 3])), float(np.linalg.norm(q))


def test_later_step_norms_against_the_librarys_own_poses(small):
    guesses = E.batch_guesses()
    off = small.run_all(ALL6, guesses, E.OUTER, None, key="mixed")
    poses = {k: small.run_all(ALL6, guesses, k, None, key="mixed")["res"]["T"] for k in range(1, E.OUTER)}
    poses[E.OUTER] = off["res"]["T"]
    worst_t = worst_r = 0.0
    for i in range(6):
        for k in range(1, E.OUTER):
            t, r = _motion_norms(poses[k][i], poses[k + 1][i])
            worst_t = max(worst_t, abs(t - float(off["steps"][i]["step_translation"][k])))
            worst_r = max(worst_r, abs(r - float(off["steps"][i]["step_rotation"][k])))
    print(f"worst |recorded - from poses|, iterations 1..{E.OUTER - 1}: translation {worst_t:.3e}, rotation {worst_r:.3e}")
    assert worst_t <= 5e-6 and worst_r <= 5e-6          # above that it would be a finding, not a bar to widen
    assert worst_t <= STEP_FROM_POSES_BAR_T and worst_r <= STEP_FROM_POSES_BAR_R


# ------------------------------------------------------------------------------------------------------------ 3. the contract
@pytest.mark.parametrize("shortcut", [True, False])
def test_contract_six_pairs(small, shortcut):
    """shortcut off: every cloud is projected (the finder's images of slot 0 exist after the batch and are compared)"""
    _shortcut(small.ctx, shortcut)
    try:
        ks, on = check_contract(small, ALL6, E.batch_guesses(), E.CONTRACT, E.OUTER, key=("mixed" if shortcut else "mixed-projected"))
        free = _stops(small.run_all(ALL6, E.batch_guesses(), E.OUTER, None, key=("mixed" if shortcut else "mixed-projected"))["steps"], E.LOOSE, E.OUTER)
    finally:
        _shortcut(small.ctx, True)
    print("k* =", ks, " without min_iterations:", free)
    assert len(set(ks)) >= 3 and E.OUTER in ks
    assert any(f < E.CONTRACT[2] and k == E.CONTRACT[2] for f, k in zip(free, ks))       # a pair held by min_iterations
    assert ks[0] < E.OUTER                                                                # the pair of slot 0 froze
    assert (on["images"] is not None) == (not shortcut)


def test_contract_may_stop_after_the_first_iteration(small):
    """min_iterations 0 and epsilons the first step of the odometry pairs meets in rotation only, plus a loose translation: pairs stop at 1, where
    the reference's own index image may not stand in for the first projection"""
    guesses = E.batch_guesses()
    ks, _ = check_contract(small, ALL6, guesses, (1.0, 1.5e-3, 0), E.OUTER, key="mixed")
    print("k* =", ks)
    assert 1 in ks and max(ks) > 1
    ks, _ = check_contract(small, ALL6, [np.eye(4, dtype=np.float32)] * 6, (1.0, 1.0, 0), E.OUTER, key="identity")     # identity guesses: the shortcut's case
    assert ks == [1] * 6


def test_contract_32_pairs_in_sub_batches_of_8_on_two_streams(small):
    idx = [i % 6 for i in range(32)]
    kinds = ("identity", "odometry", "far")
    guesses = [E.guess_for(E.SEEDS[i % 6], kinds[(i // 6 + i) % 3]) for i in range(32)]
    small.ctx.set_subbatch(64, 8); small.ctx.set_concurrency(2)
    try:
        ks, on = check_contract(small, idx, guesses, E.CONTRACT, E.OUTER, key="sub8", slot0=16)
    finally:
        small.ctx.set_subbatch(64, 64); small.ctx.set_concurrency(4)
    print("k* =", ks)
    assert len(set(ks)) >= 3 and E.OUTER in ks and min(ks) == E.CONTRACT[2]


@pytest.mark.parametrize("idx", [[3], [3, 1, 4]])
def test_contract_one_and_three_pairs(small, idx):
    """k_solve_update keeps the host's copy of the state itself: a freezing pair writes its pose there when it freezes"""
    g = E.batch_guesses()
    ks, on = check_contract(small, idx, [g[i] for i in idx], E.CONTRACT, E.OUTER, key="few")
    assert ks[0] < E.OUTER and (len(idx) == 1 or E.OUTER in ks)
    assert (on["images"] is not None) == (len(idx) == 1)


def test_contract_three_vga_pairs():
    """150 workgroups per pair: the throughput shape of the fused pass; default (sym6) clouds from raw frames"""
    from g2o_frontend_amd import api
    from test_gpu_parity import gpu_objects
    rows, cols, _, _, _ = case_params("vga")
    ctx = api.Context(0, rows, cols, 8)
    try:
        _, converter, aligner = gpu_objects(ctx, "vga")
        raw = [make_depth_pair("vga", s)[3:5] for s in E.VGA_SEEDS]
        refs = [api.Cloud(ctx, rows * cols) for _ in raw]; curs = [api.Cloud(ctx, rows * cols) for _ in raw]
        converter.computeBatch(refs + curs, [r for r, _ in raw] + [c for _, c in raw], raw_scale=0.001)
        rig = Rig(ctx, aligner, refs, curs)
        guesses = [E.guess_for(0, "identity"), E.guess_for(1, "odometry"), E.guess_for(2, "far")]
        ks, _ = check_contract(rig, [0, 1, 2], guesses, E.LOOSE, E.OUTER, key="vga")
        print("k* =", ks)
        assert len(set(ks)) >= 2 and min(ks) < E.OUTER
    finally:
        ctx.close()


def test_contract_17x65_injected_pair():
    """uploaded clouds (no index image of their own: both clouds are projected), one partial tile"""
    import align_clouds as A
    from g2o_frontend_amd import api
    case = A.mixed_case(17, 65, "small")
    ctx = api.Context(0, case.rows, case.cols, 2)
    try:
        aligner = A.gpu_aligner(ctx, case)
        r, c = A.gpu_clouds(ctx, case)
        rig = Rig(ctx, aligner, [r], [c])
        off = rig.run_min([0], [case.guess], E.OUTER, key="inj")
        st, sr = off["steps"][0]["step_translation"], off["steps"][0]["step_rotation"]
        print("s_t", st, "s_r", sr)
        # thresholds from this pair's own trace: met for the first time in the middle of the loop
        j = 3
        setting = (float(max(st[j:].max(), st[j]) * 1.5), float(max(sr[j:].max(), sr[j]) * 1.5), 0)
        ks, on = check_contract(rig, [0], [case.guess], setting, E.OUTER, key="inj")
        print("k* =", ks)
        assert 1 <= ks[0] < E.OUTER and on["images"] is not None
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------ 4. the comparison at equality
@pytest.mark.parametrize("side", ["translation", "rotation"])
def test_epsilon_equal_to_the_recorded_norm_stops_and_one_ulp_less_does_not(small, side):
    guesses = E.batch_guesses()
    off = small.run_all(ALL6, guesses, E.OUTER, None, key="mixed")
    i = 3
    for pair in (0, 2):
        tr = off["steps"][pair]["step_" + side]
        assert (tr[:i] > tr[i]).all()                                  # nothing earlier meets it
        below = float(np.nextafter(tr[i], np.float32(0)))
        at, less = (float(tr[i]), E.HUGE, 0), (below, E.HUGE, 0)
        if side == "rotation":
            at, less = (E.HUGE, float(tr[i]), 0), (E.HUGE, below, 0)
        want_less = _stops(off["steps"], less, E.OUTER)
        assert _stops(off["steps"], at, E.OUTER)[pair] == i + 1 and want_less[pair] > i + 1
        got_at = small.run_min(ALL6, guesses, E.OUTER, at)
        got_less = small.run_min(ALL6, guesses, E.OUTER, less)
        assert got_at["steps"][pair]["iterations"] == i + 1 and got_at["steps"][pair]["converged"]
        assert got_at["res"]["iterations"][pair] == i + 1
        assert got_less["steps"][pair]["iterations"] == want_less[pair]
        assert [s["iterations"] for s in got_at["steps"]] == _stops(off["steps"], at, E.OUTER)


# ------------------------------------------------------------------------------------------------------------ 5. min_iterations
def test_min_iterations(small):
    guesses = E.batch_guesses()
    off = small.run_all(ALL6, guesses, E.OUTER, None, key="mixed")
    seven = small.run_min(ALL6, guesses, E.OUTER, (1.0, 1.0, 7))
    want = small.run_min(ALL6, guesses, 7, None, key="mixed")
    assert [s["iterations"] for s in seven["steps"]] == [7] * 6 and all(s["converged"] for s in seven["steps"])
    assert seven["res"].tobytes() == want["res"].tobytes()
    above = small.run_min(ALL6, guesses, E.OUTER, (1.0, 1.0, E.OUTER + 1))
    assert [s["iterations"] for s in above["steps"]] == [E.OUTER] * 6 and not any(s["converged"] for s in above["steps"])
    assert above["res"].tobytes() == off["res"].tobytes()
    at_outer = small.run_min(ALL6, guesses, E.OUTER, (1.0, 1.0, E.OUTER))          # converged in the last iteration: nothing left to skip, same bits
    assert all(s["converged"] for s in at_outer["steps"]) and at_outer["res"].tobytes() == off["res"].tobytes()


# ------------------------------------------------------------------------------------------------------------ 6. inner iterations
def test_contract_with_two_inner_iterations(small):
    """the rule is evaluated at the end of an outer iteration, on the step of its last inner iteration"""
    ks, on = check_contract(small, ALL6, E.batch_guesses(), E.LOOSE, 8, inner=2, key="inner2")
    print("k* =", ks)
    assert min(ks) < 8 and (on["res"]["iterations"] == 2 * np.array(ks)).all()


# ------------------------------------------------------------------------------------------------------------ 7. the one-submission steps
def _same_results(a, b):
    a, b = a.copy(), b.copy()
    a["total_time_ms"] = 0; b["total_time_ms"] = 0
    assert a.tobytes() == b.tobytes()


def test_one_submission_step_equals_convert_then_align_under_the_setting():
    from g2o_frontend_amd import api
    from test_gpu_parity import gpu_objects
    rows, cols, _, _, _ = case_params("small")
    ctx = api.Context(0, rows, cols, 16)
    try:
        _, converter, aligner = gpu_objects(ctx, "small")
        raw = [make_depth_pair("small", s)[3:5] for s in E.SEEDS]
        rf = [r for r, _ in raw]; cf = [c for _, c in raw]
        n = len(raw)
        mk = lambda: [api.Cloud(ctx, rows * cols) for _ in range(n)]      # noqa: E731
        refs, curs, refs2, curs2 = mk(), mk(), mk(), mk()
        guesses = E.batch_guesses()
        ctx.set_convergence(*E.CONTRACT)
        converter.computeBatch(refs + curs, rf + cf, raw_scale=0.001)
        want_rec = np.full((n, api.RECORD_FLOATS), -7.0, np.float32)
        want = aligner.alignBatchRecords(refs, curs, want_rec, first_pair_id=3, initialGuesses=guesses).copy()
        want_steps = aligner.lastSteps(0, n)
        rec = np.full((n, api.RECORD_FLOATS), -7.0, np.float32)
        got = aligner.convertAlignBatch(converter, refs2, curs2, rf, cf, raw_scale=0.001, records=rec, first_pair_id=3, initialGuesses=guesses).copy()
        got_steps = aligner.lastSteps(0, n)
        _same_results(got, want)
        assert rec.tobytes() == want_rec.tobytes()
        assert all(_same_steps(a, b) and a["converged"] == b["converged"] for a, b in zip(got_steps, want_steps))
        its = [s["iterations"] for s in got_steps]
        print("iterations", its)
        assert len(set(its)) >= 3 and min(its) == E.CONTRACT[2] and max(its) == E.OUTER
        # records only: the states come from the device when the steps are asked for
        assert aligner.convertAlignBatch(converter, refs2, curs2, rf, cf, raw_scale=0.001, records=rec, first_pair_id=3, initialGuesses=guesses, want_results=False) is None
        assert rec.tobytes() == want_rec.tobytes() and all(_same_steps(a, b) for a, b in zip(aligner.lastSteps(0, n), want_steps))
    finally:
        ctx.close()


def test_scaled_one_submission_step_equals_scaled_convert_then_align_under_the_setting():
    from g2o_frontend_amd import api, synth
    from test_gpu_scaled_batch import make_aligner, make_converter, scaled_call
    rows, cols, K, _, _ = case_params("small")
    step = 2
    orows, ocols = rows // step, cols // step
    Ks = synth.scaled_K(K, step)
    ctx = api.Context(0, rows, cols, 16)
    try:
        converter = make_converter(Ks); aligner = make_aligner(ctx, Ks, orows, ocols)
        raw = [make_depth_pair("small", s)[3:5] for s in E.SEEDS]
        rf = [r for r, _ in raw]; cf = [c for _, c in raw]
        n = len(raw)
        mk = lambda: [api.Cloud(ctx, orows * ocols) for _ in range(n)]      # noqa: E731
        refs, curs, refs2, curs2 = mk(), mk(), mk(), mk()
        ctx.set_convergence(1e-3, 1e-4, 2)
        assert scaled_call(ctx, converter.params(None), "raw", rf + cf, rows, cols, step, refs + curs) == 0
        want_rec = np.full((n, api.RECORD_FLOATS), -7.0, np.float32)
        want = aligner.alignBatchRecords(refs, curs, want_rec).copy()
        want_steps = aligner.lastSteps(0, n)
        rec = np.full((n, api.RECORD_FLOATS), -7.0, np.float32)
        got = aligner.convertAlignBatch(converter, refs2, curs2, rf, cf, raw_scale=0.001, records=rec, step=step, max_depth_cov=0.01).copy()
        _same_results(got, want)
        assert rec.tobytes() == want_rec.tobytes()
        assert all(_same_steps(a, b) and a["converged"] == b["converged"] for a, b in zip(aligner.lastSteps(0, n), want_steps))
        print("iterations", [s["iterations"] for s in want_steps])
        assert min(s["iterations"] for s in want_steps) < E.OUTER
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------ 8. the two-pass projection
def test_forced_fallback_gives_the_bits_of_the_default_path(small):
    """pwn_hip_debug_set_settle_guard(ctx, 0): every collision of a projection gives up and the library repeats the call with the two-pass
    projection (the path tests/test_projection_fault.py runs); the repeat runs under the same setting"""
    guesses = E.batch_guesses()
    L, ctx = small.ctx._L, small.ctx
    want = small.run_all(ALL6, guesses, E.OUTER, E.CONTRACT, key="mixed")
    n0 = C.c_int(0); n1 = C.c_int(0)
    ctx.check(L.pwn_hip_debug_projection_fallbacks(ctx.h, C.byref(n0)))
    ctx.check(L.pwn_hip_debug_set_settle_guard(ctx.h, 0))
    try:
        got = small.run_all(ALL6, guesses, E.OUTER, E.CONTRACT)
    finally:
        ctx.check(L.pwn_hip_debug_set_settle_guard(ctx.h, 4096))
    ctx.check(L.pwn_hip_debug_projection_fallbacks(ctx.h, C.byref(n1)))
    assert n1.value - n0.value == 3                                   # the three alignment calls of run_all were each repeated
    for f in ("res", "scores", "stats", "rec72", "rec64"):
        assert got[f].tobytes() == want[f].tobytes(), f
    assert all(_same_steps(a, b) and a["converged"] == b["converged"] for a, b in zip(got["steps"], want["steps"]))
    assert len({s["iterations"] for s in got["steps"]}) >= 3


# ------------------------------------------------------------------------------------------------------------ 9. priors
def test_priors_with_the_setting_enabled_are_refused_and_touch_nothing(small):
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import Prior
    from test_gpu_scaled_batch import flat_bytes
    ctx, L, aligner = small.ctx, small.ctx._L, small.aligner
    ref, cur = small.refs[0], small.curs[0]
    p = small.setup(E.OUTER, 1, E.LOOSE)
    before = (flat_bytes(ref).tobytes(), flat_bytes(cur).tobytes())
    pr = (Prior * 1)()
    pr[0].kind = 0
    for k in range(4):
        pr[0].mean[5 * k] = 1.0; pr[0].reference_transform[5 * k] = 1.0
    for k in range(6):
        pr[0].information[7 * k] = 10.0
    res = api.AlignResult()
    C.memset(C.byref(res), 0xAB, C.sizeof(res))
    try:
        assert L.pwn_hip_align_with_priors(ctx.h, C.byref(p), ref.h, cur.h, 1, pr, C.byref(res)) == INVALID
        assert bytes(res) == b"\xab" * C.sizeof(res)
        assert (flat_bytes(ref).tobytes(), flat_bytes(cur).tobytes()) == before
        # no priors: the batch path, which honours the setting
        ctx.check(L.pwn_hip_align_with_priors(ctx.h, C.byref(p), ref.h, cur.h, 0, None, C.byref(res)))
        assert res.iterations < E.OUTER and small.aligner.lastSteps()[0]["converged"]
        # the mirror raises
        aligner.setReferenceCloud(ref); aligner.setCurrentCloud(cur)
        aligner.addRelativePrior(np.eye(4, dtype=np.float32), np.eye(6, dtype=np.float32) * 10.0)
        with pytest.raises(api.PwnHipError) as e:
            aligner.align()
        assert e.value.code == INVALID
        ctx.clear_convergence()
        assert aligner.align()["iterations"] == E.OUTER               # off again: the call runs, one pair of pwn_hip_align_batch_priors
        single = aligner.lastSteps()[0]                               # ... and leaves its step traces
        assert single["iterations"] == E.OUTER and len(single["step_translation"]) == E.OUTER
        assert np.all(single["step_translation"] > 0) and np.all(single["step_rotation"] > 0)
        # bit for bit the traces n = 1 of the batch call leaves for the same pair and prior
        prior = (0, np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), np.eye(6, dtype=np.float32) * 10.0)
        aligner.alignBatch([ref], [cur], priors=[[prior]])
        assert _same_steps(single, aligner.lastSteps()[0])
    finally:
        aligner.clearPriors(); ctx.clear_convergence()


# ------------------------------------------------------------------------------------------------------------ 10. the mirrors
def test_python_mirror_single_alignment(small):
    a = small.aligner
    a.setOuterIterations(E.OUTER); a.setInnerIterations(1)
    a.setReferenceCloud(small.refs[3]); a.setCurrentCloud(small.curs[3]); a.setInitialGuess(np.eye(4, dtype=np.float32))
    try:
        full = a.align(statistics=True)
        s = a.lastSteps()[0]
        k = E.stop_iteration(s["step_translation"], s["step_rotation"], E.LOOSE, E.OUTER)
        assert s["iterations"] == E.OUTER and not s["converged"] and k < E.OUTER
        small.ctx.set_convergence(*E.LOOSE[:2])
        got = a.align(images=True, statistics=True)
        omega = a.omega().copy()
        assert got["iterations"] == k and a.lastSteps()[0]["converged"] and a.lastSteps()[0]["iterations"] == k
        images = [x.copy() for x in (a.correspondenceFinder().referenceIndexImage(), a.correspondenceFinder().referenceDepthImage())]
        small.ctx.clear_convergence()
        a.setOuterIterations(k)
        want = a.align(images=True, statistics=True)
        assert np.array_equal(got["T"].view(np.uint32), want["T"].view(np.uint32)) and np.array_equal(got["chi2"].view(np.uint32), want["chi2"].view(np.uint32))
        assert np.array_equal(omega.view(np.uint32), a.omega().view(np.uint32))
        assert np.array_equal(images[0], a.correspondenceFinder().referenceIndexImage())
        assert np.array_equal(images[1].view(np.uint32), a.correspondenceFinder().referenceDepthImage().view(np.uint32))
        assert not np.array_equal(full["T"].view(np.uint32), got["T"].view(np.uint32))
    finally:
        small.ctx.clear_convergence(); a.setOuterIterations(E.OUTER)


def test_cpp_mirror_check_tool_builds_and_finds_no_difference(tmp_path):
    from g2o_frontend_amd import api, build
    from test_gpu_parity import gpu_objects
    build.build_tools()
    rows, cols, K, _, _ = case_params("small")
    ctx = api.Context(0, rows, cols, 8)
    try:
        _, converter, aligner = gpu_objects(ctx, "small")
        raw = [make_depth_pair("small", s)[3:5] for s in E.SEEDS]
        n = len(raw)
        refs = [api.Cloud(ctx, rows * cols) for _ in range(n)]; curs = [api.Cloud(ctx, rows * cols) for _ in range(n)]
        converter.computeBatch(refs + curs, [r for r, _ in raw] + [c for _, c in raw], raw_scale=0.001)
        guesses = E.batch_guesses()
        ctx.set_convergence(*E.CONTRACT)
        res = aligner.alignBatch(refs, curs, initialGuesses=guesses, raw=True)
        steps = aligner.lastSteps(0, n)
    finally:
        ctx.close()
    assert len({s["iterations"] for s in steps}) >= 3
    path = os.path.join(str(tmp_path), "early_stop.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<6i2f4f", n, rows, cols, E.OUTER, 1, E.CONTRACT[2], E.CONTRACT[0], E.CONTRACT[1], *[float(np.float32(k)) for k in K]))
        for r, c in raw:
            f.write(np.ascontiguousarray(r, np.uint16).tobytes()); f.write(np.ascontiguousarray(c, np.uint16).tobytes())
        for T in guesses:
            f.write(_cm(T).tobytes())
        for r, s in zip(res, steps):
            st = np.zeros(api._lib.MAX_ITERATIONS, np.float32); sr = np.zeros(api._lib.MAX_ITERATIONS, np.float32)
            st[:s["iterations"]] = s["step_translation"]; sr[:s["iterations"]] = s["step_rotation"]
            f.write(np.asarray(r["T"], np.float32).tobytes())
            f.write(struct.pack("<i", int(r["iterations"]))); f.write(np.float32(r["error"]).tobytes())
            f.write(struct.pack("<3i", int(r["inliers"]), s["iterations"], int(s["converged"])))
            f.write(st.tobytes()); f.write(sr.tobytes())
    exe = os.path.join(ROOT, "tools", "pwn_hip_early_stop_check")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 differences" in r.stdout
