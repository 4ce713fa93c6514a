"""pwn_hip_cloud_add and pwn_hip_merge read their sizes from the device's word while their grids come from the host's bound (one kernel set with
the mapping step).  A used cloud -- capacity 640, 600 points that would merge, then replaced by a smaller content through the public calls, so
that stale records lie behind it -- against a fresh cloud with the same content: same sizes, same collapsed indices, same bytes.  An add that
fills its destination exactly and the merge behind it against the oracle; an add refused one point beyond the capacity.  Inputs:
tests/scene_clouds.py, checked on the CPU in tests/test_scene_sizes_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_clouds as S      # noqa: E402
from test_gpu_scene_clouds import STORAGES, same_snapshot      # noqa: E402

pytestmark = pytest.mark.gpu
CAPACITY_ERROR = 6


@pytest.fixture(scope="module")
def devices():
    from g2o_frontend_amd import api
    made = {s: api.Context(device=0, max_rows=S.ROWS, max_cols=S.COLS, max_batch=1, omega_storage=s) for s in STORAGES}
    yield {s: S.DeviceSide(c) for s, c in made.items()}
    for c in made.values():
        c.close()


def used_and_fresh(dev, content):
    """(cloud A, cloud B) with the same content: A held the junk first, B is new"""
    junk = S.junk_case()
    a = dev.cloud(junk["arrays"], junk["gauss"], capacity=S.JUNK_CAPACITY)
    assert a.size() == a.numGaussians() == S.JUNK_N
    a.upload(*[content["arrays"][k] for k in S.CLOUD_KEYS]); dev.set_gaussians(a, content["gauss"])
    b = dev.cloud(content["arrays"], content["gauss"], capacity=S.JUNK_CAPACITY)
    assert a.size() == b.size() == a.numGaussians() == b.numGaussians() == content["n"]
    return a, b


def same_bytes(a, b, stats, what):
    """every downloaded array and the whole Gaussian vector of two device clouds"""
    assert a.size() == b.size() and a.numGaussians() == b.numGaussians(), what
    x, y = a.arrays(stats=stats), b.arrays(stats=stats)
    for k in x:
        assert x[k].tobytes() == y[k].tobytes(), (what, k)
    x, y = a.gaussians(), b.gaussians()
    for k in S.GAUSS_KEYS:
        assert x[k].tobytes() == y[k].tobytes(), (what, "gaussians", k)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("n", S.USED_SIZES)
def test_merge_of_a_used_cloud_equals_the_fresh_one(devices, storage, n):
    dev = devices[storage]
    case = S.mirrored_case(n)
    a, b = used_and_fresh(dev, case)
    ka, cola = dev.merge(a, case["cfg"]); kb, colb = dev.merge(b, case["cfg"])
    assert ka == kb == n - n // 2 and np.array_equal(cola, colb) and np.array_equal(cola, case["expect"])
    same_bytes(a, b, False, "merge n=%d" % n)
    assert a.numGaussians() == n                                            # never resized


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("fewer", (0, 3))
@pytest.mark.parametrize("m", S.USED_SOURCES)
@pytest.mark.parametrize("n", S.USED_SIZES)
def test_add_into_a_used_cloud_equals_the_fresh_one(devices, storage, n, m, fewer):
    """an m-point source with m, or m - 3, Gaussians"""
    dev = devices[storage]
    a, b = used_and_fresh(dev, S.mirrored_case(n))
    src = S.add_source(n=m, seed=50 + m)
    ng = max(m - fewer, 0)
    s = dev.cloud(src["arrays"], S.head_gauss(src["gauss"], ng))
    assert s.size() == m and s.numGaussians() == ng
    dev.add(a, s, S.T_A); dev.add(b, s, S.T_A)
    assert a.size() == n + m and a.numGaussians() == n + ng
    same_bytes(a, b, True, "add n=%d m=%d gaussians=%d" % (n, m, ng))
    assert s.size() == m and s.numGaussians() == ng                         # the source is not modified


@pytest.mark.parametrize("storage", STORAGES)
def test_add_that_fills_the_destination_then_merge(devices, oracle, storage):
    """k + m == capacity, against the oracle after each call"""
    dev, orc = devices[storage], S.OracleSide(oracle)
    dst, src = S.mirrored_case(257), S.sizes_case(259, True)
    k, m = dst["n"], src["n"]
    od, os_ = orc.cloud(dst["arrays"], dst["gauss"]), orc.cloud(src["arrays"], src["gauss"])
    gd, gs = dev.cloud(dst["arrays"], dst["gauss"], capacity=k + m), dev.cloud(src["arrays"], src["gauss"])
    orc.add(od, os_, S.T_FILL); dev.add(gd, gs, S.T_FILL)
    assert gd.size() == k + m == gd.numGaussians()
    same_snapshot(orc.snapshot(od), dev.snapshot(gd), "exact fill, add", sym6=storage == "sym6")
    ok, ocol = orc.merge(od, S.CFG); gk, gcol = dev.merge(gd, S.CFG)
    assert gk == ok == gd.size() and ok < k + m and np.array_equal(gcol, ocol) and gd.numGaussians() == k + m
    same_snapshot(orc.snapshot(od), dev.snapshot(gd), "exact fill, merge", sym6=storage == "sym6")


@pytest.mark.parametrize("storage", STORAGES)
def test_add_beyond_the_capacity_is_refused(devices, storage):
    """k + m == capacity + 1: PWN_HIP_ERR_CAPACITY, and the destination is untouched byte for byte, Gaussians included"""
    from g2o_frontend_amd import api
    dev = devices[storage]
    dst, src = S.mirrored_case(257), S.add_source(n=256, seed=50 + 256)
    gd, gs = dev.cloud(dst["arrays"], dst["gauss"], capacity=257 + 256 - 1), dev.cloud(src["arrays"], src["gauss"])
    before, gauss = gd.arrays(stats=False), gd.gaussians()
    ctx = dev.ctx
    assert ctx._L.pwn_hip_cloud_add(ctx.h, gd.h, gs.h, api._ptr(api._colmajor(S.T_A, 4))) == CAPACITY_ERROR
    assert gd.size() == 257 and gd.numGaussians() == 257
    after, gauss_after = gd.arrays(stats=False), gd.gaussians()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    for k in S.GAUSS_KEYS:
        assert gauss[k].tobytes() == gauss_after[k].tobytes(), k
    dev.add(gd, dev.cloud(S.add_source(n=255, seed=5)["arrays"]), S.T_A)      # one point fewer fits, and the refusal left the cloud usable
    assert gd.size() == 257 + 255
