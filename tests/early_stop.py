"""Inputs and model of the "stop when converged" tests (include/pwn_hip.h: pwn_hip_ctx_set_convergence).

The inputs are the project's synthetic pairs (g2o_frontend_amd.synth.make_pair) under the reference's two configurations; a batch mixes
identity guesses with the kind of guess the closer hands over (an odometry pose with its z translation zeroed, pwn_matcher_base.cpp:114).

The model is the rule itself, on recorded step norms: after outer iteration i (0-based) a pair stops iff i + 1 >= min_iterations and both norms
are <= their epsilon; a NaN never passes; a pair that never stops runs outer_iterations.
"""
import numpy as np

from conftest import case_params, make_depth_pair

F32 = np.float32

SEEDS = (0, 1, 2, 3, 4, 5)                 # the six pairs of the mixed batch, 120 x 160
VGA_SEEDS = (0, 1, 2)
OUTER = 10

# (translation_epsilon, rotation_epsilon, min_iterations)
LOOSE = (1e-3, 1e-4, 0)                    # a millimetre: seeds 0-5 from the identity stop after 5, 6, 5, 4, 4, 4 iterations (CPU oracle)
TIGHT = (2e-5, 9e-7, 0)                    # seed 0 does not get there in ten iterations (its last rotation step: 1.25e-6), the others stop after 7 to 10;
                                           # chosen from the oracle's table so that no deciding norm lies within 5 % of its epsilon
CONTRACT = (1e-3, 1e-4, 4)                 # the mixed batch (BATCH_GUESSES) under LOOSE stops after 5, 10 (never), 5, 3, 4, 3: min_iterations = 4 holds two pairs
HUGE = 3.0e38


def guess_for(seed, kind):
    """kind "identity"; "odometry": the pair's true pose, a little off, z translation zeroed -- the aligner starts next to the solution;
    "far": the true pose composed with a decimetre / 0.05 step -- it starts further away than the identity"""
    from g2o_frontend_amd import synth
    if kind == "identity":
        return np.eye(4, dtype=F32)
    T = synth.pair_pose(seed)
    if kind == "odometry":
        T = T @ synth.v2t(np.array([0.002, -0.001, 0.0015, 0.0005, -0.0004, 0.0006]))
        T[2, 3] = 0.0
        return T.astype(F32)
    if kind == "far":
        return (T @ synth.v2t(np.array([0.10, -0.08, 0.06, 0.05, -0.04, 0.03]))).astype(F32)
    raise KeyError(kind)


# the mixed batch: three pairs from the identity, three with the closer's kind of guess
BATCH_GUESSES = ("identity", "far", "identity", "odometry", "identity", "odometry")


def batch_guesses(seeds=SEEDS, kinds=BATCH_GUESSES):
    return [guess_for(s, k) for s, k in zip(seeds, kinds)]


def frames(name, seeds):
    """[(reference depth, current depth)] float32 metres of the seeded pairs of conftest's case `name`"""
    out = []
    for s in seeds:
        ref, cur, _, _, _ = make_depth_pair(name, s)
        out.append((ref, cur))
    return out


def step_norms(dx):
    """(s_t, s_r) of a step as the library records them: fp32, every product rounded on its own, sums left to right, correctly rounded root"""
    d = np.asarray(dx, F32)
    st = np.sqrt(F32(F32(d[0] * d[0]) + F32(d[1] * d[1])) + F32(d[2] * d[2]))
    sr = np.sqrt(F32(F32(d[3] * d[3]) + F32(d[4] * d[4])) + F32(d[5] * d[5]))
    return F32(st), F32(sr)


def stop_iteration(step_t, step_r, setting, outer_iterations):
    """k*: outer iterations a pair with these recorded norms runs under `setting` = (eps_t, eps_r, min_iterations)"""
    eps_t, eps_r, min_it = F32(setting[0]), F32(setting[1]), int(setting[2])
    for i in range(min(outer_iterations, len(step_t))):
        if i + 1 >= min_it and F32(step_t[i]) <= eps_t and F32(step_r[i]) <= eps_r:
            return i + 1
    return outer_iterations


def oracle_step_trace(O, ap, oref, ocur):
    """(s_t[i], s_r[i]) of every outer iteration of the CPU oracle's alignment (inner_iterations = 1): the norms of ldlt(H + 1001 I) \\ (-b)"""
    o = O.align(ap, oref, ocur)
    st, sr = [], []
    for it in o["iterations"]:
        H = (it["H"].astype(F32) + F32(1.0) * np.eye(6, dtype=F32)).astype(F32)
        H = (H + F32(1000.0) * np.eye(6, dtype=F32)).astype(F32)
        dx = O.ldlt_solve6(H, -it["b"])
        a, b = step_norms(dx)
        st.append(a); sr.append(b)
    return np.array(st, F32), np.array(sr, F32), o


def oracle_pair(O, name, seed, guess=None, **over):
    """the oracle's clouds and aligner parameters of a seeded pair"""
    rows, cols, K, conv, alig = case_params(name)
    ref, cur, _, _, _ = make_depth_pair(name, seed)
    cp = O.converter_params(K=K, **conv)
    oref, _, _ = O.convert(cp, ref); ocur, _, _ = O.convert(cp, cur)
    a = dict(alig); a.update(over)
    ap = O.aligner_params(rows, cols, K=K, initial_guess=guess, accumulate_fp64=1, **a)
    return ap, oref, ocur
