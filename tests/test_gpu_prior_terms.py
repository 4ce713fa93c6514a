"""k_prior_terms as shipped (pwn_hip_debug_prior_terms_eval) on the injected (invT, prior) items of tests/prior_cases.py against the host side of
the same text (pwn_hip_prior_terms): every record word for word.

Comparison rule (prior_cases.words_equal): bit equality per word; two NaNs are equal whatever their sign and payload; the valid flags are equal."""
import ctypes as C

import numpy as np
import pytest

import prior_cases as pc

pytestmark = pytest.mark.gpu


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _run(ctx, invTs, lists):
    """the hook on pairs (invT, [priors]) -> [total, 44] uint32"""
    from g2o_frontend_amd import _lib
    n = len(invTs)
    first = np.zeros(n + 1, np.int32); first[1:] = np.cumsum([len(q) for q in lists])
    total = int(first[n])
    arr = (_lib.Prior * max(total, 1))()
    for j, prior in enumerate([p for q in lists for p in q]):
        arr[j] = pc.prior_struct(prior)
    T = np.ascontiguousarray(np.stack([np.asarray(t, np.float32).T.reshape(-1) for t in invTs]))
    out = np.full((max(total, 1), 44), 0xDEADBEEF, np.uint32)
    ctx.check(ctx._L.pwn_hip_debug_prior_terms_eval(ctx.h, n, _vp(T), _vp(first), arr, _vp(out)))
    return out[:total]


def _assert_equal(got, want, what):
    eq = pc.words_equal(got, want)
    assert eq.all(), (what, np.argwhere(~eq)[:6], got[~eq][:4], want[~eq][:4])


@pytest.fixture(scope="module")
def ctx():
    from g2o_frontend_amd import api
    c = api.Context(0, 120, 160, 4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def everything():
    its = pc.all_items()
    want = np.stack([pc.host_terms(invT, prior) for _, invT, prior, _ in its])
    return its, want


def test_every_item_in_one_launch(ctx, everything):
    """the generator's full list, one prior per pair, one launch of a few thousand workgroups through a context made for 4 pairs"""
    its, want = everything
    got = _run(ctx, [invT for _, invT, _, _ in its], [[prior] for _, _, prior, _ in its])
    assert got.shape == want.shape and len(its) > 2000
    _assert_equal(got, want, "one prior per pair")
    classes = {c: [pc.outcome(w) for w in got].count(c) for c in ("finite", "nonfinite", "refused")}
    print(classes)
    assert all(classes.values())


@pytest.mark.parametrize("k", [1, 2, 3])
def test_lists_of_priors_per_pair(ctx, k):
    """k priors per pair at the pair's one transform, in list order; with pairs that carry none in between"""
    pairs = pc.lists(k, 65, seed=3)
    invTs, lists = [], []
    for i, (invT, priors) in enumerate(pairs):
        invTs.append(invT); lists.append(priors)
        if i % 7 == 3:
            invTs.append(invT); lists.append([])
    want = np.stack([pc.host_terms(invT, p) for invT, q in zip(invTs, lists) for p in q])
    _assert_equal(_run(ctx, invTs, lists), want, k)


def test_mixed_lists_with_refused_and_nonfinite_priors(ctx, everything):
    """lists of 0 .. 3 priors from every family against one transform each: a refused prior in front of a valid one leaves that one's record alone"""
    its, _ = everything
    rng = np.random.default_rng(11)
    invTs, lists = [], []
    for _ in range(130):
        k = int(rng.integers(0, 4))
        picks = [its[int(j)] for j in rng.integers(0, len(its), k)]
        invTs.append(its[int(rng.integers(0, len(its)))][1]); lists.append([p[2] for p in picks])
    want = np.stack([pc.host_terms(invT, p) for invT, q in zip(invTs, lists) for p in q])
    got = _run(ctx, invTs, lists)
    _assert_equal(got, want, "mixed")
    assert {pc.outcome(w) for w in got} == {"finite", "nonfinite", "refused"}


def test_bad_arguments_are_status_codes(ctx):
    from g2o_frontend_amd import _lib
    invT = np.eye(4, dtype=np.float32).reshape(1, 16)
    arr = (_lib.Prior * 1)(pc.prior_struct(pc.items("identity", 1)[0][1]))
    out = np.full((1, 44), 7, np.uint32)
    L = ctx._L
    ok = np.array([0, 1], np.int32)
    assert L.pwn_hip_debug_prior_terms_eval(ctx.h, 1, _vp(invT), _vp(ok), arr, _vp(out)) == 0 and out[0, 42] == 1
    out[:] = 7
    for first in (np.array([1, 1], np.int32), np.array([0, -1], np.int32)):
        assert L.pwn_hip_debug_prior_terms_eval(ctx.h, 1, _vp(invT), _vp(first), arr, _vp(out)) == 1
    assert L.pwn_hip_debug_prior_terms_eval(ctx.h, 1, None, _vp(ok), arr, _vp(out)) == 1
    assert L.pwn_hip_debug_prior_terms_eval(ctx.h, 1, _vp(invT), None, arr, _vp(out)) == 1
    assert L.pwn_hip_debug_prior_terms_eval(ctx.h, 1, _vp(invT), _vp(ok), None, _vp(out)) == 1
    arr[0].kind = 2
    assert L.pwn_hip_debug_prior_terms_eval(ctx.h, 1, _vp(invT), _vp(ok), arr, _vp(out)) == 1
    assert (out == 7).all()
    assert L.pwn_hip_debug_prior_terms_eval(ctx.h, 0, None, _vp(np.array([0], np.int32)), None, None) == 0
