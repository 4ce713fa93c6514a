"""tests/statistics_systems.py held to its claims with the oracle alone (no GPU), and the product's host statistics -- the text the device kernel
k_pair_statistics expands too -- against the oracle on the same systems."""
import collections
import ctypes as C

import numpy as np
import pytest

import statistics_systems as S

N = 200


@pytest.fixture(scope="module")
def classified(oracle):
    """family -> (H, T, oracle words [N, 44], outcome per system), computed once"""
    out = {}
    for fam in S.FAMILIES:
        H, T = S.systems(fam, N)
        w = np.stack([S.oracle_words(oracle, H[i], T[i]) for i in range(N)])
        out[fam] = (H, T, w, [S.outcome(w[i]) for i in range(N)])
    return out


def test_every_family_reaches_the_outcome_class_it_is_named_for(classified):
    total = collections.Counter()
    for fam, (_, _, _, classes) in classified.items():
        c = collections.Counter(classes)
        total.update(c)
        print(fam, dict(c))
        main = S.FAMILIES[fam][1]
        if main is not None:
            assert c[main] >= 20, (fam, dict(c))
    # the NaN rule of the comparison must not be what lets a broken kernel pass: enough systems are finite in every word
    assert total["finite"] >= 0.4 * sum(total.values()), dict(total)
    for fam in ("jtj", "jtj_x100", "jtj_x1e4", "diagonal", "tiny_offdiag", "pivot_swap"):
        assert collections.Counter(classified[fam][3])["finite"] == N, fam
    assert collections.Counter(classified["huge"][3])["zero"] == N and collections.Counter(classified["zero"][3])["nonfinite"] == N


def test_the_special_paths_are_taken(classified):
    """Counted, not assumed: the dropped and the kept singular value, the skipped Jacobi rotation, the row swap of the inverse, an infinity."""
    H, _, w, classes = classified["sv_dropped"]
    assert sum(S.drops_unit_eigenvalue(H[i]) for i in range(N)) == N
    H, _, w, classes = classified["sv_kept"]
    assert sum(S.drops_unit_eigenvalue(H[i]) for i in range(N)) == 0 and classes.count("finite") >= 20
    for fam in ("sv_dropped", "sv_kept"):      # the unconstrained direction is there, exactly: a zero row and column of H
        H = classified[fam][0]
        assert all(np.any((np.abs(H[i]).sum(axis=0) == 0)) for i in range(N))
    H = classified["tiny_offdiag"][0]
    assert all(0 < abs(H[i, 0, 1]) < 1e-30 and H[i, 0, 1] == H[i, 1, 0] and abs(H[i, 0, 2]) > 1 for i in range(N))
    assert all(not np.any(H[i] - np.diag(np.diag(H[i]))) for H in [classified["diagonal"][0]] for i in range(N))
    _, _, w, classes = classified["pivot_swap"]
    assert sum(S.swaps_rows(w[i, :36].reshape(6, 6).T) for i in range(N)) >= 20
    assert sum(S.swaps_rows(w[i, :36].reshape(6, 6).T) for i in range(N) if classified["jtj"][3][i] == "finite" for w in [classified["jtj"][2]]) == 0
    assert sum(int(np.any(np.isinf(classified[fam][2]))) for fam in classified) > 0          # an infinity: the rule's third clause is exercised
    assert any(np.isinf(w).any() for w in classified["near_pi"][2])


def test_comparison_rule():
    nan_a = np.array([0x7fc00000, 0xffc00001], np.uint32).view(np.float32); nan_b = np.array([0xffc00000, 0x7fa00000], np.uint32).view(np.float32)
    assert S.words_equal(nan_a, nan_b).all()
    assert not S.words_equal(np.float32([np.nan]), np.float32([1.0])).any() and not S.words_equal(np.float32([1.0]), np.float32([np.nan])).any()
    assert not S.words_equal(np.float32([np.inf]), np.float32([-np.inf])).any() and S.words_equal(np.float32([np.inf]), np.float32([np.inf])).all()
    assert not S.words_equal(np.float32([0.0]), np.float32([-0.0])).any()
    assert not S.words_equal(np.float32([1.0]), np.nextafter(np.float32([1.0]), np.float32(2))).any()


def test_product_host_statistics_match_the_oracle_on_every_family(classified):
    """pwn_hip_compute_statistics on all 15 x 200 systems under the comparison rule: the shared host / device text keeps the oracle's bits on the
    host, NaN and infinity cases included."""
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    for fam, (H, T, want, _) in classified.items():
        for i in range(N):
            Hc = np.ascontiguousarray(H[i].T.reshape(-1)); Tc = np.ascontiguousarray(T[i].T.reshape(-1))
            got = np.empty(44, np.float32); tr, rr = C.c_float(0), C.c_float(0)
            L.pwn_hip_compute_statistics(Hc.ctypes.data_as(C.c_void_p), Tc.ctypes.data_as(C.c_void_p), got[36:].ctypes.data_as(C.c_void_p),
                                         got.ctypes.data_as(C.c_void_p), C.byref(tr), C.byref(rr))
            got[42] = tr.value; got[43] = rr.value
            eq = S.words_equal(got, want[i])
            assert eq.all(), (fam, i, np.where(~eq)[0][:8], got[~eq][:4], want[i][~eq][:4])
