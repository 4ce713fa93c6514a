"""The SE(3) prior terms on the host (pwn_hip_prior_terms: the text of pwn_stats.h through SerialTeam), no GPU: the families of
tests/prior_cases.py reach what they claim, the terms agree with the float64 model where that is well conditioned, and adding them to an H, b is
what prior_accumulate (pwn_stats.h: the host statement of the addition the step on the device makes) does, bit for bit and in list order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import prior_cases as pc
from test_capi_cpu import ROOT, declared_symbols

# fp32 text against the float64 model (numpy_reference_model.prior_terms), relative to the largest entry of the float64 term.  Measured here with
# the host text over the compared families (2268 items less the zero information matrices): worst |Hp - Hp64| / max|Hp64| = 1.50e-3 (branch_z),
# worst |bp - bp64| / max|bp64| = 1.59e-3 (branch_x); the motion families stay below 1.6e-4.  The bar is that times 4: the numeric Jacobians
# divide an fp32 difference (a few 6e-8 on entries of size 1, more where the quaternion is extracted far from the identity) by 2e-3, and how the
# roundings line up depends on the draw.
HP_BAR = 6.0e-3
BP_BAR = 6.4e-3
# Families compared in Hp only (identity, motion_1e-7): e itself is at the rounding of the products behind X (entries of size 1 at 6e-8, four
# products), so bp = J^T Omega' e is all noise relative to itself.  Its error is bounded through Hp = J^T Omega' J instead: |dbp| <= 6 max|Hp| |J^-1 de|,
# with J ~ I and |de| <= 1e-6.
BP_ABS_FACTOR = 6e-6


@pytest.fixture(scope="module")
def evaluated():
    """every item of the generator with its host record, computed once"""
    return [(fam, invT, prior, info, pc.host_terms(invT, prior)) for fam, invT, prior, info in pc.all_items()]


def test_symbols_are_declared_prototyped_and_exported():
    from g2o_frontend_amd import _lib
    names = declared_symbols()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in ("pwn_hip_prior_terms", "pwn_hip_align_batch_priors", "pwn_hip_debug_prior_terms_eval"):
        assert sym in names, sym + " is not declared in include/"
        assert sym in _lib.PROTOTYPES, sym + " has no ctypes prototype"
        assert hasattr(L, sym), sym + " is not exported"
    boundary = open(os.path.join(ROOT, "include", "pwn_hip.h")).read()
    assert "pwn_hip_pair_priors" in boundary and "pwn_hip_debug_prior_terms_eval" not in boundary
    assert C.sizeof(_lib.PairPriors) == 2 * C.sizeof(C.c_void_p)


def test_the_generator_is_a_few_thousand_items_of_every_kind_and_matrix():
    its = pc.all_items()
    assert 2000 <= len(its) <= 5000
    for fam in pc.FAMILIES:
        mine = [(p[0], info) for f, _, p, info in its if f == fam]
        assert {k for k, _ in mine} == {0, 1} and {i for _, i in mine} == set(pc.INFORMATION), fam
    assert all(np.array_equal(invT[3], [0, 0, 0, 1]) for _, invT, _, _ in its)


def test_every_family_reaches_its_outcome(evaluated):
    for fam, (_, cls, _) in pc.FAMILIES.items():
        got = [pc.outcome(w) for f, _, _, _, w in evaluated if f == fam]
        if cls is None:      # near pi: both outcomes occur, none other
            assert set(got) == {"finite", "refused"}, (fam, set(got))
        else:
            assert set(got) == {cls}, (fam, {g: got.count(g) for g in set(got)})
    for _, _, _, _, w in evaluated:      # a refused prior hands back zeros
        Hp, bp, valid = pc.record_parts(w)
        assert valid in (0, 1) and (valid or (not Hp.any() and not bp.any()))


def test_every_family_takes_its_branch_of_t2v(evaluated):
    taken = {}
    for fam, invT, prior, _, _ in evaluated:
        if fam in pc.BRANCH_OF:
            taken.setdefault(fam, set()).add(pc.t2v_branch(pc.error_rotation(invT, prior)))
    assert taken == {f: {b} for f, b in pc.BRANCH_OF.items()}
    assert {b for s in taken.values() for b in s} == {0, 1, 2, 3}


def test_near_pi_is_within_1e_3_of_pi(evaluated):
    for fam, invT, prior, _, _ in evaluated:
        if fam == "near_pi":
            R = pc.error_rotation(invT, prior).astype(np.float64)
            angle = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
            assert np.pi - angle < 1.2e-3


def test_zero_information_gives_zero_terms(evaluated):
    n = 0
    for fam, _, _, info, w in evaluated:
        if info == "zero" and pc.FAMILIES[fam][1] == "finite":
            Hp, bp, valid = pc.record_parts(w)
            assert valid == 1 and not Hp.any() and not bp.any(), fam
            n += 1
    assert n > 100


def test_terms_agree_with_the_float64_model(evaluated):
    """Excluded by name: near_pi (the differences of the numeric Jacobians straddle the sign fix of t2v at w ~ 0), refused and nonfinite_mean
    (nothing to compare), and the zero information matrix (exact zeros, the test above).  identity and motion_1e-7 are compared in Hp, and in bp
    absolutely."""
    import numpy_reference_model as M
    worst = {}
    for fam, invT, prior, info, w in evaluated:
        mode = pc.FAMILIES[fam][2]
        if mode is None or info == "zero":
            continue
        Hp, bp, valid = pc.record_parts(w)
        H64, b64 = M.prior_terms(prior[0], prior[1], prior[3], invT, prior[2])
        eH = np.abs(Hp - H64).max() / np.abs(H64).max()
        eb = np.abs(bp - b64).max() / (np.abs(b64).max() if mode == "Hb" else np.abs(H64).max())
        k = worst.setdefault((fam, mode), [0.0, 0.0])
        k[0] = max(k[0], eH); k[1] = max(k[1], eb)
    for (fam, mode), (eH, eb) in sorted(worst.items()):
        print(f"{fam:18s} {mode:2s} Hp {eH:.3g}  bp {eb:.3g}")
    assert {f for f, _ in worst} == {f for f, (_, _, m) in pc.FAMILIES.items() if m}
    for (fam, mode), (eH, eb) in worst.items():
        assert eH <= HP_BAR, (fam, eH)
        assert eb <= (BP_BAR if mode == "Hb" else BP_ABS_FACTOR), (fam, mode, eb)


_ACCUMULATE_PROGRAM = r'''
#include <cstdio>
#include <vector>
#include "pwn_stats.h"
using namespace pwnhip;
// in: per list  k, invT[16], H[36], b[6], then k x { kind, mean[16], referenceTransform[16], information[36] }  (floats);  out: per list H[36], b[6]
int main(int argc, char** argv) {
  FILE* in = std::fopen(argv[1], "rb"); FILE* out = std::fopen(argv[2], "wb");
  float k;
  while (std::fread(&k, 4, 1, in) == 1) {
    float T[16], H[36], b[6];
    if (std::fread(T, 4, 16, in) != 16 || std::fread(H, 4, 36, in) != 36 || std::fread(b, 4, 6, in) != 6) return 1;
    for (int j = 0; j < (int)k; ++j) {
      float q[69];
      if (std::fread(q, 4, 69, in) != 69) return 1;
      PriorHost pr;
      pr.kind = (int)q[0]; pr.mean = mat4_from(q + 1);
      pr.invReference = pr.kind == 1 ? iso_inverse(mat4_from(q + 17)) : mat4_identity();
      for (int i = 0; i < 36; ++i) pr.information[i] = q[33 + i];
      prior_accumulate(pr, mat4_from(T), H, b);
    }
    std::fwrite(H, 4, 36, out); std::fwrite(b, 4, 6, out);
  }
  std::fclose(out);
  return 0;
}
'''


def test_adding_the_terms_is_prior_accumulate_in_list_order(tmp_path):
    """prior_accumulate itself -- the host statement of "terms, then add in list order", compiled for the host into a stand-alone program with the library's
    flags -- on lists of 1, 2 and 3 priors, against H[i] + Hp[i], b[i] + bp[i] of pwn_hip_prior_terms added in list order in float32.  The lists
    mix magnitudes (information 1e-3 .. 1e12), so the reversed order gives other bits for some: the check is order-sensitive."""
    from g2o_frontend_amd import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = tmp_path / "accumulate.hip"; exe = tmp_path / "accumulate"
    src.write_text(_ACCUMULATE_PROGRAM)
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC") and not f.startswith("--offload-arch")]
    subprocess.check_call([hipcc, "--cuda-host-only"] + flags + ["-I", os.path.join(ROOT, "g2o_frontend_amd", "csrc"), "-o", str(exe), str(src)])
    rng = np.random.default_rng(5)
    cases = [pair for k in (1, 2, 3) for pair in pc.lists(k, 12)]
    # a list with a refused prior in the middle: skipped, the others added
    refused = pc.items("refused", 1)[0][1]
    cases.append((cases[-1][0], [cases[-1][1][0], refused, cases[-1][1][1]]))
    H0 = []; stream = []
    for invT, priors in cases:
        J = rng.normal(size=(50, 6)) * np.array([30, 30, 30, 60, 60, 60])
        H = (J.T @ J).astype(np.float32); b = (J.T @ rng.normal(size=50)).astype(np.float32)
        H0.append((H, b))
        stream += [np.float32([len(priors)]), invT.T.reshape(-1), H.T.reshape(-1), b]
        for kind, mean, reft, info in priors:
            stream += [np.float32([kind]), mean.T.reshape(-1), reft.T.reshape(-1), np.asarray(info, np.float32).T.reshape(-1)]
    np.concatenate([np.asarray(s, np.float32) for s in stream]).tofile(tmp_path / "in.bin")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", np.float32).reshape(len(cases), 42)

    def added(invT, priors, H, b):
        H = H.T.reshape(-1).copy(); b = b.copy()
        for prior in priors:
            Hp, bp, valid = pc.record_parts(pc.host_terms(invT, prior))
            if valid:
                H = H + Hp.T.reshape(-1); b = b + bp
        return np.concatenate([H, b])

    order_matters = 0
    for (invT, priors), (H, b), g in zip(cases, H0, got):
        want = added(invT, priors, H, b)
        assert np.array_equal(want.view(np.uint32), g.view(np.uint32)), len(priors)
        if len(priors) > 1 and not np.array_equal(added(invT, priors[::-1], H, b).view(np.uint32), g.view(np.uint32)):
            order_matters += 1
    assert order_matters > 0
    # the refused prior added nothing
    assert np.array_equal(got[-1].view(np.uint32), added(cases[-1][0], [cases[-1][1][0], cases[-1][1][2]], *H0[-1]).view(np.uint32))
