"""The inputs of tests/test_gpu_scene_sizes.py on the CPU: the oracle alone gives what their construction says (tests/scene_clouds.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_clouds as S      # noqa: E402


@pytest.mark.parametrize("n", S.USED_SIZES)
def test_oracle_merge_of_the_mirrored_content(oracle, n):
    case = S.mirrored_case(n)
    S.check_placement(oracle, case["arrays"]["points"], case["r"], case["c"])
    c = S.oracle_cloud(oracle, case["arrays"], case["gauss"])
    k, col = S.oracle_merge(oracle, c, case["cfg"])
    assert np.array_equal(col, case["expect"]) and k == n - n // 2 == len(c) and c.num_gaussians() == n
    merged = np.nonzero(col != np.arange(n))[0]
    assert len(merged) == n // 2
    if n == 257:                          # a pair whose members lie in different blocks of 256
        assert (merged // 256 != col[merged] // 256).any()
    if n == 256:                          # one block: pairs in different waves of it
        assert (merged // 64 != col[merged] // 64).sum() >= 64


def test_oracle_merge_of_the_junk(oracle):
    """the records a used cloud keeps behind its content would merge, and all of them lie inside the view"""
    case = S.junk_case()
    S.check_placement(oracle, case["arrays"]["points"], case["r"], case["c"])
    c = S.oracle_cloud(oracle, case["arrays"], case["gauss"])
    k, col = S.oracle_merge(oracle, c, case["cfg"])
    assert np.array_equal(col, case["expect"]) and k == S.JUNK_N // 2
    assert S.JUNK_N - 257 > 256 and S.JUNK_N <= S.JUNK_CAPACITY      # a third block of junk behind the largest content


def test_oracle_exact_fill(oracle):
    """the add of the exact-fill case appends every point of the source, and the merge behind it merges some of them"""
    side = S.OracleSide(oracle)
    dst, src = S.mirrored_case(257), S.sizes_case(259, True)
    d = side.cloud(dst["arrays"], dst["gauss"]); s = side.cloud(src["arrays"], src["gauss"])
    side.add(d, s, S.T_FILL)
    assert len(d) == 257 + 259 == d.num_gaussians()
    k, col = side.merge(d, S.CFG)
    assert k == len(d) < 257 + 259 and len(col) == 257 + 259 and d.num_gaussians() == 257 + 259
    assert ((col[257:] >= 0) & (col[257:] < 257)).any()              # points of the source merge into points the destination held
