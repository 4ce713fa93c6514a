"""The consensus validation of closures on the host (pwn_hip_validate_relation, pwn_hip_validate_relations_host) against the independent float64
model and the closed forms of tests/consensus_cases.py; the ABI; the refusals; the orientation finding (docs/parity.md).  No GPU.

The bar between the host's float32 error matrices and the model's: |delta| <= 2^-23 |value| + 1e-30 per entry -- one float ulp for the
double-to-float rounding behind two implementations of sqrt and atan2 that differ by less than 1e-15.  A decision isIn is compared wherever
the model's value lies further than that bar from its threshold; counters and decisions in every case in which no entry lies inside the bar."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import consensus_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pwn_hip_default_consensus_params", "pwn_hip_validate_relation", "pwn_hip_validate_relations_host", "pwn_hip_validate_relations")
_CACHE = {}


def evaluated(case):
    """(host result, model) of a case, computed once"""
    if case["name"] not in _CACHE:
        _CACHE[case["name"]] = (cc.run_host(case), cc.model(case))
    return _CACHE[case["name"]]


@pytest.fixture(scope="module")
def cases():
    return cc.all_cases()


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_symbols_are_declared_prototyped_and_exported():
    from g2o_frontend_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pwn_hip.h")).read(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.PROTOTYPES and hasattr(L, name), name
    assert "PWN_HIP_CONSENSUS_MAX_RELATIONS 8192" in src


def test_struct_size_and_defaults(tmp_path):
    from g2o_frontend_amd import _lib
    prog = '#include <stdio.h>\n#include "pwn_hip.h"\nint main(void) { printf("%zu %d\\n", sizeof(pwn_hip_consensus_params), PWN_HIP_CONSENSUS_MAX_RELATIONS); return 0; }\n'
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    size, cap = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).decode().split()]
    assert size == C.sizeof(_lib.ConsensusParams) and cap == 8192
    p = _lib.ConsensusParams()
    _lib.lib().pwn_hip_default_consensus_params(C.byref(p))
    assert np.float32(p.inlier_translational_threshold) == np.float32(0.25)
    assert np.float32(p.inlier_rotational_threshold) == np.float32(np.float32(15.0) * np.pi / np.float32(180.0))          # map_closer.cpp:64
    assert p.min_times_checked == 5
    assert (np.float32(p.inlier_translational_threshold), np.float32(p.inlier_rotational_threshold)) == (cc.THR_T, cc.THR_R)


def test_refusals_without_a_device():
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    case = cc.cluster_case(5)
    before = cc.run_host(case)
    assert before["rc"] == 0
    untouched = lambda r: (all(np.array_equal(r[k], np.asarray(a, np.int32)) for k, a in zip(("times_checked", "cum_inlier", "cum_outlier_times"), case["counters"]))
                           and (r["decisions"] == -7).all() and (r["te"] == -1).all() and (r["re"] == -1).all())
    for params in ((0.25, 2.2, 5), (0.25, 0.0, 5), (0.25, -0.1, 5), (0.25, float("nan"), 5), (0.0, 0.26, 5), (float("nan"), 0.26, 5)):
        r = cc.run_host(case, params=params)
        assert r["rc"] == 1 and untouched(r), params
    assert cc.run_host(case, params=(0.25, np.float32(2 * np.pi / 3 - 1e-6), 5))["rc"] == 0           # the upper end of the range is allowed
    # null required arguments
    n = case["n"]; tc = cc.colmajor(case["tc"]); cnt = np.zeros(n, np.int32); dec = np.zeros(n, np.int32)
    p = cc.params_struct(case["params"])
    full = [C.byref(p), n, cc.vp(tc), cc.vp(tc), cc.vp(tc), None, cc.vp(cnt), cc.vp(cnt), cc.vp(cnt), cc.vp(dec), None, None, None]
    assert L.pwn_hip_validate_relations_host(*full) in (0, 1)                                        # callable with the optional ones NULL
    for k in (0, 2, 3, 4, 6, 7, 8, 9):
        args = list(full); args[k] = None
        assert L.pwn_hip_validate_relations_host(*args) == 1, k
    # n == 0 is a no-op, n beyond the cap a capacity error
    args = list(full); args[1] = 0
    assert L.pwn_hip_validate_relations_host(*args) == 0
    args[1] = 8193
    assert L.pwn_hip_validate_relations_host(*args) == 6
    assert b"PWN_HIP_CONSENSUS_MAX_RELATIONS" in L.pwn_hip_last_error_string(None)
    # the device call without a context
    assert L.pwn_hip_validate_relations(None, C.byref(p), n, cc.vp(tc), cc.vp(tc), cc.vp(tc), None, 0, None, cc.vp(cnt), cc.vp(cnt), cc.vp(cnt), cc.vp(dec), None, None) == 1


# ------------------------------------------------------------------------------------------------------------------------ host against model
def test_single_columns_equal_the_matrices_bit_for_bit(cases):
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    for case in cases:
        n = case["n"]
        if n > 129 and case["family"] not in ("rotation", "exact"):
            continue
        h, _ = evaluated(case)
        tc, to, tr = cc.colmajor(case["tc"]), cc.colmajor(case["to"]), cc.colmajor(case["tr"])
        te = np.empty(n, np.float32); re = np.empty(n, np.float32)
        for i in range(n):
            L.pwn_hip_validate_relation(n, cc.vp(tc), cc.vp(to), cc.vp(tr), cc.vp(case["flags"]), i, cc.vp(te), cc.vp(re))
            assert np.array_equal(te.view(np.uint32), np.ascontiguousarray(h["te"][:, i]).view(np.uint32)), (case["name"], i)
            assert np.array_equal(re.view(np.uint32), np.ascontiguousarray(h["re"][:, i]).view(np.uint32)), (case["name"], i)


def test_host_matrices_decisions_and_counters_against_the_model(cases):
    worst = {}
    inside_total = {}
    for case in cases:
        h, m = evaluated(case)
        assert h["rc"] == 0 and m["empty_column"] == -1, case["name"]
        for key in ("te", "re"):
            a, b = h[key].astype(np.float64), m[key].astype(np.float64)
            d = np.abs(a - b)
            bar = cc.BAR * np.abs(b) + 1e-30
            assert (d <= bar).all(), (case["name"], key, float(d.max()), int(np.argmax(d - bar)))
            rel = np.where(b != 0, d / np.maximum(np.abs(b), 1e-300), 0.0).max()
            fam = worst.setdefault(case["family"], {"te": 0.0, "re": 0.0, "te_abs": 0.0, "re_abs": 0.0})
            fam[key] = max(fam[key], float(rel)); fam[key + "_abs"] = max(fam[key + "_abs"], float(d.max()))
        inside = cc.inside_bar(m, case["params"])
        assert np.array_equal(h["is_in"][~inside], m["is_in"][~inside]), case["name"]
        t = inside_total.setdefault(case["family"], [0, 0]); t[0] += int(inside.sum()); t[1] += inside.size
        if not inside.any():
            for k in ("times_checked", "cum_inlier", "cum_outlier_times", "decisions"):
                assert np.array_equal(h[k].astype(np.int64), m[k]), (case["name"], k)
    for fam in sorted(worst):
        print("family %-9s worst |delta| te %.3g (rel %.3g)  re %.3g (rel %.3g)  entries inside the bar %d of %d"
              % (fam, worst[fam]["te_abs"], worst[fam]["te"], worst[fam]["re_abs"], worst[fam]["re"], inside_total[fam][0], inside_total[fam][1]))
    # the cap: over the realistic cases at most 0.1 % of the entries lie inside the bar (the generator's seeds meet it on the model alone)
    assert inside_total["realistic"][0] <= 1e-3 * inside_total["realistic"][1]


def test_exact_family_holds_its_closed_form_bits_and_decisions(cases):
    seen = {"at": 0, "above": 0, "below": 0, "in": 0}
    for case in cases:
        if case["family"] != "exact":
            continue
        h, m = evaluated(case)
        want = cc.closed_form_exact(case)
        assert np.array_equal(h["te"].view(np.uint32), want.view(np.uint32)), case["name"]
        assert np.array_equal(m["te"].view(np.uint32), want.view(np.uint32)), case["name"]
        assert (h["re"].view(np.uint32) == 0).all() and (m["errors"]["nvec"] == 0).all(), case["name"]      # every rotation is exactly the identity: n == 0
        host_in = h["is_in"]
        n = case["n"]
        if "g" in case and case["g"].any():
            for b in range(0, n, 7):
                for j, i, what in cc.EXACT_EDGES:
                    if b + max(i, j) >= n:
                        continue
                    v = h["te"][b + j, b + i]; seen[what] += 1
                    if what == "at": assert v == np.float32(0.25) and not host_in[b + j, b + i]                   # 0.25f itself is out
                    if what == "above": assert v == np.nextafter(np.float32(0.25), np.float32(1)) and not host_in[b + j, b + i]
                    if what == "below": assert v == np.nextafter(np.float32(0.25), np.float32(0)) and host_in[b + j, b + i]   # one ulp below is in
                    if what == "in": assert v == np.float32(0.0625) and host_in[b + j, b + i]
            at = np.abs(m["te"].astype(np.float64) - 0.25) <= 2.0 ** -25
            if n >= 63:
                assert at.sum() >= 10, (case["name"], int(at.sum()))                                          # coverage floor: entries at the threshold
                assert (m["errors"]["nvec"] == 0).sum() - n >= n                                               # n == 0, the diagonal not counted
        else:
            assert (h["te"].view(np.uint32) == 0).all() and host_in.all()                                       # all-zero translations
    assert min(seen.values()) >= 50, seen


def test_rotation_ladder_switches_exactly_once_and_the_branches_are_covered(cases):
    for case in cases:
        if case["family"] != "rotation":
            continue
        h, m = evaluated(case)
        labels = np.array(case["labels"])
        host_in = h["is_in"]
        for a in range(4):
            rungs = np.flatnonzero(labels == "ladder%d" % a)
            if len(rungs) < len(cc.LADDER_K):
                continue
            for col in (host_in[rungs, 0], host_in[0, rungs], m["is_in"][rungs, 0]):        # te(k, 0) = R_k^T and te(0, k) = R_k; increasing angle
                assert col[0] and not col[-1], (case["name"], a)
                assert (np.diff(col.astype(int)) <= 0).all() and (np.diff(col.astype(int)) != 0).sum() == 1, (case["name"], a, col)
            ang = h["re"][rungs, 0].astype(np.float64)
            assert (np.diff(ang) >= 0).all() and abs(ang[len(rungs) // 2] - float(cc.THR_R)) < 1e-7
        e = m["errors"]
        off = ~np.eye(case["n"], dtype=bool)
        if case["carries_all"]:
            for b in range(4):
                assert (e["branch"] == b).sum() >= 20, (case["name"], b)
            assert ((e["w"] < 0) & (e["branch"] > 0)).sum() >= 20 and (e["w"] == 0).sum() >= 1, case["name"]
            assert ((e["nvec"] == 0) & off).sum() >= case["n"], case["name"]
            for lab, want in (("deg90", np.pi / 2), ("deg120-", 2 * np.pi / 3 - 1e-6), ("deg120+", 2 * np.pi / 3 + 1e-6), ("deg180x", np.pi), ("deg180y", np.pi),
                              ("deg180z", np.pi), ("deg180s", np.pi), ("deg179.999", np.deg2rad(179.999))):
                k = int(np.flatnonzero(labels == lab)[0])
                assert abs(float(h["re"][k, 0]) - want) <= 4e-7 and abs(float(h["re"][0, k]) - want) <= 4e-7, (case["name"], lab, float(h["re"][k, 0]))
                assert not host_in[k, 0]
            z = np.flatnonzero(labels == "zero")
            assert (h["re"][np.ix_(z, z)].view(np.uint32) == 0).all() and (h["re"][z, 0].view(np.uint32) == 0).all()


def test_vote_edges_and_clusters_have_their_closed_forms(cases):
    deltas, arrivals = set(), set()
    for case in cases:
        if case["family"] not in ("votes", "clusters"):
            continue
        h, m = evaluated(case)
        t, ci, co, dec = cc.closed_form_clusters(case)
        for got in (h, m):
            assert np.array_equal(np.asarray(got["times_checked"], np.int64), t) and np.array_equal(np.asarray(got["cum_inlier"], np.int64), ci), case["name"]
            assert np.array_equal(np.asarray(got["cum_outlier_times"], np.int64), co) and np.array_equal(np.asarray(got["decisions"], np.int64), dec), case["name"]
            assert np.array_equal(got["c"], case["group_size"]), case["name"]
        if case["family"] == "votes":
            minT = case["params"][2]
            assert np.array_equal(ci - co, case["delta"]), case["name"]
            decided = t >= minT
            assert (dec[~decided] == 0).all() and (dec[decided & (case["delta"] > 0)] == 1).all() and (dec[decided & (case["delta"] <= 0)] == 2).all()
            if case["n"] >= 12:
                deltas |= set(case["delta"][decided].tolist()); arrivals |= set((case["arriving"] - minT).tolist())
    assert deltas == {-1, 0, 1} and arrivals == {-2, -1, 0, 3}


# ------------------------------------------------------------------------------------------------------------------------ the finding
def _accepted(r):
    return np.asarray(r["decisions"]) == 1


@pytest.mark.parametrize("distinct", [False, True])
def test_orientation_finding_on_64_relations(distinct):
    """The rule of validateRelation is a consistency check only when a relation's transform maps current -> other as other^-1 * current; the
    closers store current^-1 * other.  Literal orientation (the reference): a relation's only inliers are the relations on its own node pair, so
    none of the good relations gathers a majority.  Consistent orientation (every flag set): exactly the good ones are accepted.
    64 relations on partitions of 5 and 7 nodes must share node pairs (35 < 64), and two good relations on one pair agree in any orientation;
    `distinct` runs the same scenario on 8 x 8 nodes with one relation per pair, where every column has exactly one inlier, itself."""
    # Two relations on DIFFERENT node pairs can agree by accident in the literal orientation (the drift cancels out of its error, what is left
    # depends on the node poses alone); the seeds are ones at which the model shows no such accident, so that the counts are exact.
    kw = dict(nodes=(8, 8), distinct_pairs=True, seed=33) if distinct else dict(seed=11)
    lit = cc.realistic_case(64, 0.3, consistent=False, **kw)
    con = cc.realistic_case(64, 0.3, consistent=True, **kw)
    good = lit["good"]
    assert good.sum() == 45 and np.array_equal(good, con["good"])
    pair_of = np.array([a * 100 + b for a, b in lit["pairs"]])
    same_pair = pair_of[:, None] == pair_of[None, :]
    for run in (cc.run_host, lambda c: cc.model(c)):
        r = run(lit)
        assert not _accepted(r)[good].any() and not _accepted(r).any()
        c, is_in = r["c"], r["is_in"]
        assert not (is_in & ~same_pair).any()                       # no inlier off a relation's own node pair
        if distinct:
            assert (np.asarray(c) == 1).all()
        else:
            assert np.array_equal(np.asarray(c), (same_pair & good[:, None] & good[None, :] | np.eye(64, dtype=bool)).sum(0))
        r = run(con)
        assert np.array_equal(_accepted(r), good)
        c = r["c"]
        print("distinct pairs %s: literal accepts %d of %d good, consistent accepts %d of %d good and %d of %d bad; consistent c of a good relation %d"
              % (distinct, 0, good.sum(), _accepted(r)[good].sum(), good.sum(), _accepted(r)[~good].sum(), (~good).sum(), int(np.asarray(c)[good].min())))


def test_realistic_cases_accept_exactly_the_good_relations_when_consistent(cases):
    for case in cases:
        if case["family"] != "realistic" or case["n"] < 63 or case["flags"][0] == 0:
            continue
        h, m = evaluated(case)
        if case["name"].find("_o60_") < 0:                            # with 60 % outliers the good ones are a minority of the votes but still agree
            assert np.array_equal(_accepted(h), case["good"]), case["name"]
        assert not _accepted(h)[~case["good"]].any(), case["name"]


# ------------------------------------------------------------------------------------------------------------------------ "no inliers"
def test_a_nan_pose_is_the_no_inliers_error_and_changes_nothing():
    from g2o_frontend_amd import _lib
    case = cc.nan_case()
    h, m = cc.run_host(case), cc.model(case)
    assert m["empty_column"] == case["nan_at"] == h["empty_column"] and h["rc"] == 1
    assert ("column %d" % case["nan_at"]).encode() in _lib.lib().pwn_hip_last_error_string(None)
    for k, a in zip(("times_checked", "cum_inlier", "cum_outlier_times"), case["counters"]):
        assert h[k].tobytes() == np.asarray(a, np.int32).tobytes()
    assert (h["decisions"] == -7).all()
    ok = cc.run_host(cc.exact_case(65, seed=2))
    assert ok["rc"] == 0 and ok["empty_column"] == -1
