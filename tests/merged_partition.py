"""Inputs and numpy model of the merged closure (Merger2::mergeDepthImage, pwn_tracker2/merger2.cpp:75-101; PwnCloserWithMerger,
pwn_tracker2/pwn_closer_with_merger.cpp:108-224) for tests/test_merged_partition_cpu.py and tests/test_gpu_merged_partition.py.

The model has two forms that must agree bit for bit: merge_images (vectorised float32) and merge_images_literal (the reference's loop,
pixel by pixel).  Every float operation is a numpy float32 operation (IEEE, rounded separately); the three comparisons against the
reference's double literals are made in float64.

Inputs: `natural_case` -- seeded room frames along a trajectory, converted with the oracle and projected into the first frame's view;
`injected_case` -- planes written directly, every special depth value and every threshold of the loop on both of its sides, each on a
fresh pixel (out == 0) and on a filled one."""
import functools

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
K_SMALL = (65.6, 65.6, 39.5, 29.5)              # the 60 x 80 natural case
MIN_DISTANCE, MAX_DISTANCE = 0.01, 6.0          # the merger's projector (PointProjector's defaults, pointprojector.cpp:9-10)


# ---------------------------------------------------------------------------------------------------------------- the model
def merge_images(out, weights, images, variant=None):
    """n successive Merger2::mergeDepthImage calls -> (out, weights, overlap[n], points, stats).  stats counts the branches taken.
    variant: None = the reference's arithmetic; "fma" / "fma2" = the first / the second product contracted into the sum (a float64 product of
    two float32 values is exact, so the sum is rounded once, up to the double rounding of the final cast), "rcp" = the division as a
    multiplication by the reciprocal -- the wrong roundings a kernel could have; stats counts the fusions each of them rounds differently (from the same
    operands), to show that the inputs tell them apart."""
    out = np.array(out, F); w = np.array(weights, F)
    overlap, points = [], 0
    st = dict(first=0, nearer=0, fused=0, beyond=0, near_threshold=0, fma_differs=0, fma2_differs=0, rcp_differs=0)
    with np.errstate(all="ignore"):
        for d in images:
            d = np.asarray(d, F)
            d64 = d.astype(np.float64)
            sel = (d64 > 0.1) & (d64 < 10000)                                    # merger2.cpp:80
            peso = F(1) / d                                                      # :82
            diff = d - out
            fresh = out == 0
            rep = sel & (fresh | (diff.astype(np.float64) < -.00003))            # :84
            fus = sel & ~rep & (np.abs(diff).astype(np.float64) < .2)            # :91
            somma = w + peso                                                     # :93
            num = out * w + d * peso                                             # :94
            num_fma = (out.astype(np.float64) * w.astype(np.float64) + (d * peso).astype(np.float64)).astype(F)
            num_fma2 = ((out * w).astype(np.float64) + d.astype(np.float64) * peso.astype(np.float64)).astype(F)
            exact, fma, fma2, rcp = num / somma, num_fma / somma, num_fma2 / somma, num * (F(1) / somma)
            mean = dict(fma=fma, fma2=fma2, rcp=rcp).get(variant, exact)
            for name, wrong in (("fma", fma), ("fma2", fma2), ("rcp", rcp)):
                st[name + "_differs"] += int((fus & (bits(wrong) != bits(exact))).sum())
            st["first"] += int((rep & fresh).sum()); st["nearer"] += int((rep & ~fresh).sum())
            st["fused"] += int(fus.sum()); st["beyond"] += int((sel & ~rep & ~fus).sum())
            st["near_threshold"] += int((sel & ~fresh & (np.abs(diff.astype(np.float64) + .00003) < 1e-6)).sum())
            out = np.where(rep, d, np.where(fus, mean, out))
            w = np.where(rep, peso, np.where(fus, somma, w))
            overlap.append(int(sel.sum())); points += int(rep.sum())
    return out, w, np.array(overlap, np.int32), points, st


def merge_images_literal(out, weights, images):
    """merger2.cpp:75-101 as written, one pixel at a time -> (out, weights, overlap[n], points)"""
    out = np.array(out, F); w = np.array(weights, F)
    o, p = out.reshape(-1), w.reshape(-1)
    overlap, points = [], 0
    with np.errstate(all="ignore"):
        for img in images:
            cur = np.asarray(img, F).reshape(-1)
            count = 0
            for i in range(cur.size):
                d = cur[i]
                if float(d) > 0.1 and float(d) < 10000:
                    count += 1
                    peso = F(1) / d
                    if o[i] == 0 or float(F(d - o[i])) < -.00003:
                        points += 1
                        o[i] = d
                        p[i] = peso
                    elif float(np.abs(F(d - o[i]))) < .2:
                        somma = F(p[i] + peso)
                        o[i] = F(F(F(o[i] * p[i]) + F(d * peso)) / somma)
                        p[i] = somma
            overlap.append(count)
    return out, w, np.array(overlap, np.int32), points


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ natural input
def room_frames(seed, n, rows, cols, K):
    """float32 depth frames of the seeded room along synth.trajectory(seed, n, t_step=0.08, r_step_deg=4.0) and their camera poses"""
    from g2o_frontend_amd import synth
    from oracle import oracle as O
    poses = synth.trajectory(seed, n, t_step=0.08, r_step_deg=4.0)
    frames = [O.convert_16u_to_32f(synth.render_depth_mm(seed, poses[k], rows, cols, K, hole_stream=k)) for k in range(n)]
    return frames, poses


def converter_conf(rows):
    from oracle import oracle as O
    conf = dict(O.QVGA4_CONF_CONVERTER if rows <= 120 else O.VGA_CONF_CONVERTER)
    return conf


@functools.lru_cache(maxsize=None)
def natural_case(rows=60, cols=80, K=K_SMALL, seed=3, n=9):
    """Frames 1 .. n-1 converted with the oracle and projected into the view of frame 0 (projector k = inv(pose_k) @ pose_0) ->
    dict(frames, poses, clouds (oracle), points [k] (m_k x 4), transforms [k] (float32 4x4), planes [k] (the oracle's depth images))"""
    from oracle import oracle as O
    frames, poses = room_frames(seed, n, rows, cols, K)
    cp = O.converter_params(K, **converter_conf(rows))
    clouds, points, transforms, planes = [], [], [], []
    for k in range(1, n):
        c, _, _ = O.convert(cp, frames[k])
        T = (np.linalg.inv(poses[k]) @ poses[0]).astype(F)
        P = c.arrays()["points"]
        clouds.append(c); points.append(P); transforms.append(T)
        planes.append(O.project(K, T, MIN_DISTANCE, MAX_DISTANCE, rows, cols, P)[1])
    return dict(rows=rows, cols=cols, K=K, frames=frames, poses=poses, clouds=clouds, points=points, transforms=transforms, planes=planes, conf=cp)


# ----------------------------------------------------------------------------------------------------------- injected input
def _ulps(x, ks):
    """float32 neighbours of x: k ulps away for each k (k = 0 is x itself)"""
    out = []
    for k in ks:
        v = F(x)
        for _ in range(abs(k)):
            v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf), dtype=F)
        out.append(v)
    return out


def _depth_for_difference(base, target, k):
    """the float32 d nearest base + target, moved k ulps of d: d - base (rounded in float32, then widened) steps across `target`"""
    return _ulps(F(F(base) + F(target)), [k])[0]


REPEAT = 8          # pixels per label and branch side


def injected_labels():
    """label -> (d, out before): every special value and every threshold of merger2.cpp:80-96, fresh (out == 0) and filled"""
    lab = {}
    filled = F(1.5)
    specials = dict(zero=F(0), neg_zero=F(-0.0), negative=F(-1.25), denormal=F(1e-40), flt_max=FLT_MAX, pos_inf=F(np.inf), neg_inf=F(-np.inf),
                    nan=F(np.nan))
    for name, v in specials.items():
        lab[name + "/fresh"] = (v, F(0)); lab[name + "/filled"] = (v, filled)
    for name, x in (("lo", 0.1), ("hi", 10000)):
        for k in (-2, -1, 0, 1, 2):
            v = _ulps(F(x), [k])[0]
            lab["%s%+d/fresh" % (name, k)] = (v, F(0)); lab["%s%+d/filled" % (name, k)] = (v, filled if name == "lo" else F(9999.95))
    for k in (-2, -1, 0, 1, 2):                                   # d - out around -3e-5: only meaningful on a filled pixel; the fresh twin has out = 0
        d = _depth_for_difference(filled, -.00003, k)
        lab["nearer%+d/filled" % k] = (d, filled); lab["nearer%+d/fresh" % k] = (d, F(0))
    for sign in (1, -1):                                          # |d - out| around 0.2 on both sides of out
        for k in (-2, -1, 0, 1, 2):
            d = _depth_for_difference(filled, sign * .2, sign * k)
            lab["fuse%s%+d/filled" % ("+" if sign > 0 else "-", k)] = (d, filled); lab["fuse%s%+d/fresh" % ("+" if sign > 0 else "-", k)] = (d, F(0))
    return lab


def injected_case(rows, cols, n, seed=0):
    """n planes + pre-filled out / weights of rows x cols: plane 0 carries the labels (REPEAT pixels each when the image is large enough,
    cyclically otherwise), the later planes seeded depths around what is there so that every branch keeps being taken on every plane.
    -> dict(planes, out, weights, label_pixels)"""
    rng = np.random.default_rng(seed + 1000 * rows + cols)
    N = rows * cols
    lab = injected_labels()
    names = sorted(lab)
    out = np.zeros(N, F); w = np.zeros(N, F); p0 = np.zeros(N, F)
    label_pixels = {k: [] for k in names}
    for i in range(N):
        name = names[(i // REPEAT) % len(names)] if N >= REPEAT * len(names) else names[i % len(names)]
        d, o = lab[name]
        p0[i] = d; out[i] = o; w[i] = F(0) if o == 0 else F(1) / o
        label_pixels[name].append(i)
    planes = [p0]
    base = rng.uniform(0.3, 4.0, N).astype(F)
    for k in range(1, n):
        jitter = rng.choice(np.array([0, 1e-5, -2e-5, -4e-5, 0.05, -0.15, 0.19, 0.21, -0.5, 0.9], F), N)
        p = (base + jitter).astype(F)
        p[rng.random(N) < 0.1] = FLT_MAX                          # pixels nothing projects to
        p[rng.random(N) < 0.03] = 0
        planes.append(p)
    shape = (rows, cols)
    return dict(planes=[p.reshape(shape) for p in planes], out=out.reshape(shape), weights=w.reshape(shape), label_pixels=label_pixels)


# ------------------------------------------------------------------------------------------------ the closer's host algebra
def som_of(size):
    """int som = (int)round(size / 8) with integer division; 0 becomes 1 (pwn_closer_with_merger.cpp:134-135)"""
    return max(1, int(size) // 8)


def rejected(nonZeros, outliers, inliers, minNonZero=3000, minInliers=1000):
    """pwn_closer_with_merger.cpp:167-169, integer halves and eighths"""
    return nonZeros < minNonZero // 2 or outliers > inliers // 8 or inliers < minInliers // 2


def projector_transform(otherT, currentT, offset):
    """tr = other.T^-1 * current.T * offset in double, cast to float (:149, mergeNode :216-217)"""
    return (np.linalg.inv(np.asarray(otherT, np.float64)) @ np.asarray(currentT, np.float64) @ np.asarray(offset, np.float64)).astype(F)


def relation_transform(nodo2T, currentT, result, nodoT):
    """nodo2.T^-1 * (current.T * result * current.T^-1) * nodo.T in double (:175-188)"""
    cT = np.asarray(currentT, np.float64)
    return np.linalg.inv(np.asarray(nodo2T, np.float64)) @ ((cT @ np.asarray(result, np.float64) @ np.linalg.inv(cT)) @ np.asarray(nodoT, np.float64))


INFORMATION = np.diag([100.0, 100.0, 100.0, 1000.0, 1000.0, 1000.0])      # :196-198
