"""No-GPU side of "stop when converged" (include/pwn_hip.h: pwn_hip_ctx_set_convergence): the boundary, the model the GPU tests compare with, and
-- with the CPU oracle alone -- that the inputs of tests/test_gpu_early_stop.py cover what those tests claim: pairs that stop at different
iterations, none of them decided by a norm next to its threshold, and pairs that never get to the tight setting."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import early_stop as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pwn_hip_ctx_set_convergence", "pwn_hip_ctx_get_convergence", "pwn_hip_last_align_steps")


def test_symbols_are_declared_prototyped_and_exported():
    from g2o_frontend_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pwn_hip.h")).read(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES and hasattr(L, name), name
    for mirror in ("set_convergence", "clear_convergence", "convergence"):
        from g2o_frontend_amd import api
        assert hasattr(api.Context, mirror)
    assert hasattr(api.Aligner, "lastSteps")
    hpp = open(os.path.join(ROOT, "g2o_frontend_amd", "host", "pwn_hip.hpp")).read()
    for mirror in ("setConvergence", "clearConvergence", "convergence", "lastSteps"):
        assert re.search(r"\b%s\s*\(" % mirror, hpp), mirror


def test_the_two_structs_are_plain_c_with_the_mirrors_sizes():
    from g2o_frontend_amd import _lib
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "pwn_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(pwn_hip_convergence), sizeof(pwn_hip_align_steps), offsetof(pwn_hip_convergence, min_iterations),
         offsetof(pwn_hip_align_steps, step_translation), offsetof(pwn_hip_align_steps, step_rotation));
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"),
                               os.path.join(d, "t.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert out == [C.sizeof(_lib.Convergence), C.sizeof(_lib.AlignSteps), _lib.Convergence.min_iterations.offset, _lib.AlignSteps.step_translation.offset,
                   _lib.AlignSteps.step_rotation.offset]
    assert C.sizeof(_lib.AlignSteps) == 8 + 8 * _lib.MAX_ITERATIONS


def test_the_model():
    st = np.array([5e-2, 2e-3, 9e-4, 8e-4, 1e-5], np.float32); sr = np.array([2e-2, 5e-5, 2e-4, 9e-5, 1e-6], np.float32)
    assert E.stop_iteration(st, sr, (1e-3, 1e-4, 0), 5) == 4            # iteration 2 passes in translation only, iteration 1 in rotation only
    assert E.stop_iteration(st, sr, (1e-3, 1e-4, 5), 5) == 5            # held by min_iterations
    assert E.stop_iteration(st, sr, (1e-3, 1e-4, 9), 5) == 5            # min_iterations above outer_iterations: nobody stops
    assert E.stop_iteration(st, sr, (1e-6, 1e-7, 0), 5) == 5            # never converges
    assert E.stop_iteration(st, sr, (1.0, 1.0, 0), 5) == 1 and E.stop_iteration(st, sr, (1.0, 1.0, 1), 5) == 1
    assert E.stop_iteration(st, sr, (1.0, 1.0, 0), 0) == 0
    # the comparison is <= on the fp32 values
    assert E.stop_iteration(st, sr, (float(st[2]), 1.0, 0), 5) == 3
    assert E.stop_iteration(st, sr, (float(np.nextafter(st[2], np.float32(0))), 1.0, 0), 5) == 4
    assert E.stop_iteration(st, sr, (1.0, float(sr[1]), 0), 5) == 2
    assert E.stop_iteration(st, sr, (1.0, float(np.nextafter(sr[1], np.float32(0))), 0), 5) == 5
    # a NaN never passes
    nan = np.array([np.nan] * 5, np.float32)
    assert E.stop_iteration(nan, sr, (1.0, 1.0, 0), 5) == 5 and E.stop_iteration(st, nan, (1.0, 1.0, 0), 5) == 5
    # the norms: products rounded on their own, sums left to right
    a, b = E.step_norms(np.array([3.0, 4.0, 12.0, 1e-4, 2e-4, 2e-4], np.float32))
    assert a == np.float32(13.0) and abs(float(b) - 3e-4) < 1e-10


def _margin_ok(st, sr, setting, outer, margin=0.05):
    """no deciding norm within `margin` of its threshold: before the stop, an iteration that may stop (min_iterations) fails by a norm more than
    `margin` above its epsilon; at the stop both norms are more than `margin` below"""
    eps_t, eps_r, min_it = setting
    k = E.stop_iteration(st, sr, setting, outer)
    for i in range(k):
        if i + 1 < min_it:
            continue
        stops = st[i] <= eps_t and sr[i] <= eps_r
        if stops:
            assert i + 1 == k
            if not (st[i] < (1 - margin) * eps_t and sr[i] < (1 - margin) * eps_r):
                return False
        elif not (st[i] > (1 + margin) * eps_t or sr[i] > (1 + margin) * eps_r):
            return False
    return True


@pytest.fixture(scope="module")
def traces(oracle):
    """the oracle's step norms of the six pairs from the identity and under the mixed batch's guesses"""
    out = {}
    for label, kinds in (("identity", ("identity",) * 6), ("mixed", E.BATCH_GUESSES)):
        rows = []
        for s, kind in zip(E.SEEDS, kinds):
            ap, oref, ocur = E.oracle_pair(oracle, "small", s, guess=E.guess_for(s, kind), outer_iterations=E.OUTER)
            st, sr, _ = E.oracle_step_trace(oracle, ap, oref, ocur)
            rows.append((st, sr))
            print(label, s, kind, "s_t", " ".join("%.2e" % x for x in st), "| s_r", " ".join("%.2e" % x for x in sr))
        out[label] = rows
    return out


def test_the_steps_shrink_and_a_millimetre_stops_the_six_pairs_at_different_iterations(traces):
    ks = [E.stop_iteration(st, sr, E.LOOSE, E.OUTER) for st, sr in traces["identity"]]
    assert ks == [5, 6, 5, 4, 4, 4]
    assert len(set(ks)) >= 3
    for st, sr in traces["identity"]:
        assert st[0] > 100 * st[-1] and _margin_ok(st, sr, E.LOOSE, E.OUTER)


def test_the_mixed_batch_covers_what_the_contract_test_asserts(traces):
    free = [E.stop_iteration(st, sr, E.LOOSE, E.OUTER) for st, sr in traces["mixed"]]
    ks = [E.stop_iteration(st, sr, E.CONTRACT, E.OUTER) for st, sr in traces["mixed"]]
    assert len(set(ks)) >= 3 and E.OUTER in ks
    assert any(f < E.CONTRACT[2] and k == E.CONTRACT[2] for f, k in zip(free, ks))      # a pair held by min_iterations
    assert sum(1 for g in E.BATCH_GUESSES if g != "identity") == 3
    for st, sr in traces["mixed"]:
        assert _margin_ok(st, sr, E.CONTRACT, E.OUTER) and _margin_ok(st, sr, E.LOOSE, E.OUTER)
    # the pair at outer_iterations has not converged there either
    i = ks.index(E.OUTER)
    st, sr = traces["mixed"][i]
    assert not (st[-1] <= E.CONTRACT[0] and sr[-1] <= E.CONTRACT[1])


def test_a_pair_never_converges_under_the_tight_setting(traces):
    never = [not any(a <= E.TIGHT[0] and b <= E.TIGHT[1] for a, b in zip(st, sr)) for st, sr in traces["identity"]]
    assert any(never) and not all(never)
    for st, sr in traces["identity"]:
        assert _margin_ok(st, sr, E.TIGHT, E.OUTER)
