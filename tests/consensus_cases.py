"""Inputs for the consensus validation of closures (MapCloser::validatePartitions, reference boss_map_building/map_closer.cpp:200-253, :286-417)
and an independent float64 numpy model of it: what tests/test_consensus_cpu.py holds the host functions to and tests/test_gpu_consensus.py
feeds to the device call.

A case is a dict: name, n, tc / to / tr [n, 4, 4] float64 (the pose of a relation's node in the current partition, of its node in the other one,
and its transform), flags (int32 [n], bit 0 = invert the transform) or None, counters (times_checked, cum_inlier, cum_outlier_times: int32 [n],
what the call finds), params (translational threshold, rotational threshold, min_times_checked), and what its family knows about it.

The model is written from the reference's text and Eigen's Quaternion(Matrix3) / AngleAxis(Quaternion) (3.3), vectorised over the n x n pairs.
It follows the evaluation order the library documents -- products ((a0 b0 + a1 b1) + a2 b2), the inverse as R^T, -(R^T t) -- because the
rotational error of a pair that agrees to 1e-16 IS its rounding noise: another order gives another noise, far outside any relative bar.  Its
square root and arc tangent are numpy's own.  It shares no code with the library.

Families:
  exact      identity rotations, dyadic translations: every operation is exact, transErr is known in closed form (closed_form_exact)
  rotation   tc = to = identity, relation 0 the identity, relation k a rotation: te(k, 0) = R_k^T, te(0, k) = R_k
  votes      clusters with initial counters that land on cum_inlier == cum_outlier_times and one vote either side, times_checked around the minimum
  realistic  the drift scenario: two partitions, noisy good relations, gross outliers, in both orientations
  clusters   k groups of identical relations, mutually far apart: the counters have a closed form (closed_form_clusters)"""
import numpy as np

SIZES = (1, 2, 63, 64, 65, 128, 129, 257, 513)
THR_T = np.float32(0.25)
THR_R = np.float32(15.0 * np.pi / 180.0)
DEFAULT_PARAMS = (THR_T, THR_R, 5)
BAR = 2.0 ** -23               # one float ulp, relative: the double-to-float rounding behind two implementations of sqrt and atan2


# ---------------------------------------------------------------------------------------------------------------- the model
def _mul(A, B):
    """Isometry3d * Isometry3d on (R [..., 3, 3], t [..., 3]) pairs, broadcasting"""
    Ra, ta = A; Rb, tb = B
    shape = np.broadcast_shapes(Ra.shape, Rb.shape)
    R = np.empty(shape); t = np.empty(shape[:-1])
    for i in range(3):
        for j in range(3):
            R[..., i, j] = (Ra[..., i, 0] * Rb[..., 0, j] + Ra[..., i, 1] * Rb[..., 1, j]) + Ra[..., i, 2] * Rb[..., 2, j]
        t[..., i] = ((Ra[..., i, 0] * tb[..., 0] + Ra[..., i, 1] * tb[..., 1]) + Ra[..., i, 2] * tb[..., 2]) + ta[..., i]
    return R, t


def _inv(A):
    R, t = A
    Rt = np.swapaxes(R, -1, -2)
    ti = np.empty(t.shape)
    for i in range(3):
        ti[..., i] = -((R[..., 0, i] * t[..., 0] + R[..., 1, i] * t[..., 1]) + R[..., 2, i] * t[..., 2])
    return Rt.copy(), ti


def _split(T):
    T = np.asarray(T, np.float64)
    return T[..., :3, :3].copy(), T[..., :3, 3].copy()


def _angle(R):
    """AngleAxisd(R).angle() of Eigen 3.3 -> (angle, branch 0..3 [0 = trace > 0, 1 + i = diagonal entry i largest], w, |vec|)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        tr = (R[..., 0, 0] + R[..., 1, 1]) + R[..., 2, 2]
        pos = tr > 0
        i = np.zeros(tr.shape, int)
        i[R[..., 1, 1] > R[..., 0, 0]] = 1
        dii = np.where(i == 0, R[..., 0, 0], R[..., 1, 1])
        i[R[..., 2, 2] > dii] = 2
        branch = np.where(pos, 0, 1 + i)
        q = np.full(tr.shape + (4,), np.nan)                                   # x, y, z, w
        t = np.sqrt(tr + 1.0); s = 0.5 / t
        q0 = np.stack([(R[..., 2, 1] - R[..., 1, 2]) * s, (R[..., 0, 2] - R[..., 2, 0]) * s, (R[..., 1, 0] - R[..., 0, 1]) * s, 0.5 * t], -1)
        q[branch == 0] = q0[branch == 0]
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            t = np.sqrt(R[..., a, a] - R[..., b, b] - R[..., c, c] + 1.0); s = 0.5 / t
            qa = np.empty(tr.shape + (4,))
            qa[..., a] = 0.5 * t
            qa[..., 3] = (R[..., c, b] - R[..., b, c]) * s
            qa[..., b] = (R[..., b, a] + R[..., a, b]) * s
            qa[..., c] = (R[..., c, a] + R[..., a, c]) * s
            q[branch == 1 + a] = qa[branch == 1 + a]
        n = np.sqrt((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2])
        ang = np.where(n != 0, 2.0 * np.arctan2(n, np.abs(q[..., 3])), 0.0)
    return ang, branch, q[..., 3], n


def errors(case):
    """the two n x n error matrices in double (element [j, i]: reference relation i against relation j), and how the angle came about"""
    TC, TO, T0 = _split(case["tc"]), _split(case["to"]), _split(case["tr"])
    flags = case["flags"]
    inv = np.zeros(case["n"], bool) if flags is None else (np.asarray(flags) & 1).astype(bool)
    Ti = _inv(T0)
    TR = (np.where(inv[:, None, None], Ti[0], T0[0]), np.where(inv[:, None], Ti[1], T0[1]))
    tfix = _mul(_mul(TO, TR), _inv(TC))
    toInv, trInv = _inv(TO), _inv(TR)
    row = lambda A: (A[0][:, None], A[1][:, None])                             # index j
    col = lambda A: (A[0][None, :], A[1][None, :])                             # index i
    te = _mul(row(trInv), _mul(row(toInv), _mul(col(tfix), row(TC))))
    trans = (te[1][..., 0] * te[1][..., 0] + te[1][..., 1] * te[1][..., 1]) + te[1][..., 2] * te[1][..., 2]
    ang, branch, w, nvec = _angle(te[0])
    return dict(trans=trans, rot=ang, branch=branch, w=w, nvec=nvec)


def model(case, e=None):
    """everything validatePartitions does -> te / re (float32 [n, n], [j, i]), is_in, c, empty_column (-1: none), the counters after the call
    and the decisions (the counters unchanged and decisions None when a column is empty)"""
    e = errors(case) if e is None else e
    thrT, thrR, minTimes = case["params"]
    with np.errstate(invalid="ignore", over="ignore"):
        te = e["trans"].astype(np.float32); re = e["rot"].astype(np.float32)
        is_in = (te < np.float32(thrT)) & (np.abs(re) < np.float32(thrR))
    c = is_in.sum(0).astype(np.int64)
    tcheck, cin, cout = [np.asarray(a, np.int64).copy() for a in case["counters"]]
    out = dict(te=te, re=re, is_in=is_in, c=c, empty_column=-1, errors=e)
    if (c == 0).any():
        out.update(empty_column=int(np.argmax(c == 0)), times_checked=tcheck, cum_inlier=cin, cum_outlier_times=cout, decisions=None)
        return out
    tcheck += 1
    cin += (is_in * c[None, :]).sum(1)
    cout += (~is_in).sum(1)
    dec = np.where(tcheck < minTimes, 0, np.where(cin > cout, 1, 2))
    out.update(times_checked=tcheck, cum_inlier=cin, cum_outlier_times=cout, decisions=dec)
    return out


def inside_bar(m, params):
    """entries whose model value lies within the bar of its threshold: there the decision may differ between two correct implementations"""
    thrT, thrR, _ = params
    near = lambda v, thr: np.abs(v.astype(np.float64) - float(thr)) <= BAR * np.abs(v.astype(np.float64)) + 1e-30
    return near(m["te"], np.float32(thrT)) | near(m["re"], np.float32(thrR))


# ---------------------------------------------------------------------------------------------------------------- helpers
def rotation(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def iso(R=None, t=None):
    X = np.eye(4)
    if R is not None: X[:3, :3] = R
    if t is not None: X[:3, 3] = t
    return X


def _counters(rng, n, fresh=False):
    if fresh:
        return [np.zeros(n, np.int32) for _ in range(3)]
    return [rng.integers(0, 9, n).astype(np.int32), rng.integers(0, 50, n).astype(np.int32), rng.integers(0, 50, n).astype(np.int32)]


def _case(name, family, tc, to, tr, flags, counters, params=DEFAULT_PARAMS, **known):
    n = len(tc)
    c = dict(name=name, family=family, n=n, tc=np.ascontiguousarray(tc, np.float64), to=np.ascontiguousarray(to, np.float64),
             tr=np.ascontiguousarray(tr, np.float64), flags=None if flags is None else np.ascontiguousarray(flags, np.int32),
             counters=[np.ascontiguousarray(a, np.int32) for a in counters], params=(np.float32(params[0]), np.float32(params[1]), int(params[2])))
    c.update(known)
    return c


# ---------------------------------------------------------------------------------------------------------------- exact
# g = to.t + tr.t - tc.t of a relation; te(j, i).translation = g_i - g_j exactly.  The seven positions of a block, against position 0:
#   1: exactly 0.5 m (transErr == 0.25f: out)   2: 0.25f + one float ulp (out)   3: 0.25f - one float ulp (in)
#   4, 5, 6: 2^20 m away; 5 is 0.25 m from 4 (in), 6 is 0.5 m from 4 (out)
_EXACT_BLOCK = np.array([[0, 0, 0], [0.5, 0, 0], [0.5, 2.0 ** -13, 2.0 ** -13], [0.5 - 2.0 ** -26, 0, 0],
                         [2.0 ** 20, 0, 0], [2.0 ** 20 + 0.25, 0, 0], [2.0 ** 20 + 0.5, 0, 0]])
EXACT_EDGES = ((1, 0, "at"), (2, 0, "above"), (3, 0, "below"), (5, 4, "in"), (6, 4, "at"))       # (j, i, what) within a block


def exact_case(n, seed=0, zero=False):
    rng = np.random.default_rng(1000 + seed)
    k = np.arange(n)
    g = _EXACT_BLOCK[k % 7] + np.stack([np.zeros(n), 64.0 * (k // 7), np.zeros(n)], 1)
    if zero:
        g = np.zeros((n, 3))
    cpos = rng.integers(-512, 512, (n, 3)) / 64.0                                # dyadic, |.| < 8
    ppos = rng.integers(-512, 512, (n, 3)) / 64.0
    if zero:
        cpos = cpos * 0; ppos = ppos * 0
    opos = g - ppos + cpos
    mk = lambda t: np.stack([iso(t=v) for v in t])
    flags = None
    tr = mk(ppos)
    if seed % 2 == 1 and not zero:                                               # every other relation stored inverted, flag set
        flags = (k % 2).astype(np.int32)
        tr = mk(np.where(flags[:, None] == 1, -ppos, ppos))
    return _case("exact%s_n%d_s%d" % ("_zero" if zero else "", n, seed), "exact", mk(cpos), mk(opos), tr, flags, _counters(rng, n), g=g)


def closed_form_exact(case):
    """float32 [n, n]: transErr of every pair, from the positions alone"""
    g = case["g"]
    d = g[None, :, :] - g[:, None, :]                                            # [j, i] = g_i - g_j, exact
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- rotation
SKEW = np.array([0.3, -0.5, 0.8])
LADDER_AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), tuple(SKEW))
LADDER_K = tuple(range(-50, 51, 5))                                              # rungs of k * 1e-9 rad around the threshold


def rotation_list(n):
    """relation 0 is the identity; -> [(label, axis, angle)] for relations 1 .., most important first, truncated to n - 1"""
    L = []
    thr = float(THR_R)
    for a, ax in enumerate(LADDER_AXES):
        for k in LADDER_K:
            L.append(("ladder%d" % a, ax, thr + k * 1e-9))
    L.append(("deg90", (0, 0, 1), np.pi / 2))
    L += [("deg120-", SKEW, 2 * np.pi / 3 - 1e-6), ("deg120+", SKEW, 2 * np.pi / 3 + 1e-6)]
    L += [("deg180x", (1, 0, 0), np.pi), ("deg180y", (0, 1, 0), np.pi), ("deg180z", (0, 0, 1), np.pi), ("deg180s", SKEW, np.pi)]
    L.append(("deg179.999", SKEW, np.deg2rad(179.999)))
    m = int(np.ceil(np.sqrt(n))) + 1
    L += [("zero", (1, 0, 0), 0.0)] * m                                          # copies of relation 0: te exactly the identity, n == 0
    for deg in np.linspace(125, 175, 10):                                        # trace <= 0: each branch, w of either sign
        for dom in ((1, 0.2, -0.1), (0.15, 1, 0.2), (-0.2, 0.1, 1)):
            for sgn in (1, -1):
                L.append(("branch", sgn * np.asarray(dom, float), np.deg2rad(deg)))
    return L[:max(0, n - 1)], len(L)


def rotation_case(n, seed=0):
    rng = np.random.default_rng(2000 + seed)
    L, full = rotation_list(n)
    R = [np.eye(3)]
    labels = ["identity"]
    for lab, ax, ang in L:
        Rk = np.eye(3) if ang == 0.0 else rotation(ax, ang)
        if lab in ("deg90", "deg180x", "deg180y", "deg180z"):                    # about a coordinate axis: the exact matrix (w == 0 at 180 degrees)
            Rk = np.round(Rk)
        R.append(Rk); labels.append(lab)
    while len(R) < n:                                                            # filler: small random rotations
        R.append(rotation(rng.normal(size=3), rng.uniform(0.0, 0.2))); labels.append("filler")
    I = np.stack([np.eye(4)] * n)
    return _case("rotation_n%d_s%d" % (n, seed), "rotation", I, I.copy(), np.stack([iso(R=r) for r in R]), None, _counters(rng, n), labels=labels,
                 carries_all=(n - 1 >= full))


# ---------------------------------------------------------------------------------------------------------------- clusters, votes
def _cluster_sizes(n, k):
    base = [n // k + (1 if i < n % k else 0) for i in range(k)]
    return [s for s in base if s > 0]


def cluster_case(n, k=5, seed=0, counters=None, params=DEFAULT_PARAMS, name=None):
    """k groups of identical relations (fewer when n < k), the groups 64 m apart: per call c_i = s, cum_inlier_j += s^2, cum_outlier_times_j += n - s"""
    rng = np.random.default_rng(3000 + seed)
    sizes = _cluster_sizes(n, k)
    group = np.repeat(np.arange(len(sizes)), sizes)
    group = group[rng.permutation(n)]                                            # the members of a group are spread over the tiles
    tr = np.stack([iso(R=np.round(rotation((0, 0, 1), np.pi / 2 * (g % 4))), t=(64.0 * g, 0.5 * g, -2.0)) for g in group])      # quarter turns: exact
    tc = np.stack([iso(t=(1.0, 2.0, 0.5))] * n)
    to = np.stack([iso(t=(-3.0, 0.25, 1.0))] * n)
    s = np.asarray(sizes)[group]
    return _case(name or "clusters_n%d_k%d_s%d" % (n, k, seed), "clusters", tc, to, tr, None, _counters(rng, n) if counters is None else counters, params,
                 group=group, group_size=s)


def closed_form_clusters(case, calls=1):
    """the three counters after `calls` calls, and the decisions of the last one"""
    s = case["group_size"].astype(np.int64); n = case["n"]
    t0, i0, o0 = [np.asarray(a, np.int64) for a in case["counters"]]
    t, ci, co = t0 + calls, i0 + calls * s * s, o0 + calls * (n - s)
    dec = np.where(t < case["params"][2], 0, np.where(ci > co, 1, 2))
    return t, ci, co, dec


def vote_case(n, min_times=5, seed=0):
    """clusters whose initial counters put cum_inlier - cum_outlier_times at -1, 0, +1 after the call (0 is removed: strict >), with
    times_checked arriving at min - 2, min - 1, min and min + 3"""
    base = cluster_case(n, k=3, seed=seed, counters=[np.zeros(n, np.int32)] * 3)
    s = base["group_size"].astype(np.int64)
    k = np.arange(n)
    delta = (k % 3) - 1                                                          # cum_inlier - cum_outlier_times after the call
    gain = s * s - (n - s)                                                       # what the call adds to that difference
    start = delta - gain
    cin = np.where(start > 0, start, 0) + 7; cout = np.where(start < 0, -start, 0) + 7
    tcheck = min_times + np.array([-2, -1, 0, 3])[(k // 3) % 4]
    c = cluster_case(n, k=3, seed=seed, counters=[tcheck, cin, cout], params=(THR_T, THR_R, min_times), name="votes_min%d_n%d" % (min_times, n))
    c["family"] = "votes"; c["delta"] = delta; c["arriving"] = tcheck
    return c


# ---------------------------------------------------------------------------------------------------------------- realistic
def _random_pose(rng, spread, max_angle):
    return iso(R=rotation(rng.normal(size=3), rng.uniform(0, max_angle)), t=rng.uniform(-spread, spread, 3))


def realistic_case(n, outliers=0.3, consistent=False, seed=0, nodes=(5, 7), distinct_pairs=False):
    """Two partitions of nodes[0] (current) and nodes[1] (other) key frames.  The other partition's estimated poses carry a drift D the current
    one's do not; a good relation is the true relative pose current^-1 * other (what the closers store) with 1 cm / 3 mrad of noise, a gross
    outlier a random transform.  consistent: every flag set (the transform inverted before use), else none."""
    rng = np.random.default_rng(4000 + seed)
    nc, no = nodes
    if distinct_pairs:
        assert nc * no >= n
    # key nodes scattered over a few metres with unrelated headings (on a regular ladder of headings two neighbouring node pairs agree by accident)
    cur = [iso(R=rotation((0, 0, 1), rng.uniform(-1.2, 1.2)) @ rotation(rng.normal(size=3), 0.05), t=(rng.uniform(-3, 3), rng.uniform(-3, 3), 0.05 * rng.normal()))
           for a in range(nc)]
    oth = [iso(R=rotation((0, 0, 1), 2.5 + rng.uniform(-1.2, 1.2)) @ rotation(rng.normal(size=3), 0.05),
               t=(rng.uniform(-3, 3), 2.0 + rng.uniform(-3, 3), 0.05 * rng.normal())) for b in range(no)]
    D = iso(R=rotation((0.1, -0.2, 1.0), np.deg2rad(20.0)), t=(1.5, -0.8, 0.3))
    if distinct_pairs:
        pairs = [(p // no, p % no) for p in rng.permutation(nc * no)[:n]]
    else:
        pairs = [(int(rng.integers(nc)), int(rng.integers(no))) for _ in range(n)]
    good = np.ones(n, bool)
    good[rng.permutation(n)[:int(round(outliers * n))]] = False
    tc, to, tr = [], [], []
    for k, (a, b) in enumerate(pairs):
        tc.append(cur[a]); to.append(D @ oth[b])
        if good[k]:
            noise = iso(R=rotation(rng.normal(size=3), rng.normal() * 3e-3), t=rng.normal(size=3) * 1e-2)
            tr.append(np.linalg.inv(cur[a]) @ oth[b] @ noise)
        else:
            tr.append(_random_pose(rng, 3.0, np.pi))
    flags = np.ones(n, np.int32) if consistent else np.zeros(n, np.int32)
    name = "realistic_%s_o%d_n%d_s%d%s" % ("consistent" if consistent else "literal", int(outliers * 100), n, seed, "_distinct" if distinct_pairs else "")
    # fresh counters and min_times_checked = 1: the call's own vote decides
    return _case(name, "realistic", np.stack(tc), np.stack(to), np.stack(tr), flags, _counters(rng, n, fresh=True), (THR_T, THR_R, 1), good=good,
                 pairs=pairs)


def nan_case(n=65, where=17):
    c = exact_case(n, seed=2)
    c["name"] = "nan_n%d" % n
    c["tc"][where, 1, 3] = np.nan
    c["nan_at"] = where
    return c


def all_cases(sizes=SIZES):
    out = []
    for n in sizes:
        out.append(exact_case(n, seed=n))
        out.append(rotation_case(n))
        out.append(cluster_case(n))
        out.append(vote_case(n, 5))
        for o in (0.3, 0.45, 0.6):
            out.append(realistic_case(n, o, consistent=False, seed=n))
            out.append(realistic_case(n, o, consistent=True, seed=n))
    out.append(exact_case(64, zero=True))
    out.append(vote_case(65, 0)); out.append(vote_case(65, 1))
    return out


# ---------------------------------------------------------------------------------------------------------------- calling the library
def colmajor(T):
    """[n, 4, 4] -> [n, 16] float64, column-major as the C-ABI takes poses"""
    T = np.asarray(T, np.float64)
    return np.ascontiguousarray(T.transpose(0, 2, 1).reshape(len(T), 16))


def vp(a):
    import ctypes as C
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def params_struct(params):
    from g2o_frontend_amd import _lib
    return _lib.ConsensusParams(float(params[0]), float(params[1]), int(params[2]))


def run_host(case, matrices=True, counters=None, params=None):
    """pwn_hip_validate_relations_host -> rc, empty_column, the three counters and decisions after the call, te / re as float32 [j, i]"""
    import ctypes as C
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    n = case["n"]
    tc, to, tr = colmajor(case["tc"]), colmajor(case["to"]), colmajor(case["tr"])
    cnt = [np.ascontiguousarray(a, np.int32).copy() for a in (case["counters"] if counters is None else counters)]
    dec = np.full(n, -7, np.int32)
    te = np.full((n, n), np.float32(-1)) if matrices else None
    re = np.full((n, n), np.float32(-1)) if matrices else None
    empty = C.c_int(-5)
    p = params_struct(case["params"] if params is None else params)
    rc = L.pwn_hip_validate_relations_host(C.byref(p), n, vp(tc), vp(to), vp(tr), vp(case["flags"]), vp(cnt[0]), vp(cnt[1]), vp(cnt[2]), vp(dec), vp(te), vp(re),
                                           C.byref(empty))
    out = dict(rc=rc, empty_column=empty.value, times_checked=cnt[0], cum_inlier=cnt[1], cum_outlier_times=cnt[2], decisions=dec,
               te=None if te is None else te.T, re=None if re is None else re.T)
    if matrices:                                                                 # the votes as the matrices imply them
        with np.errstate(invalid="ignore"):
            out["is_in"] = (out["te"] < np.float32(p.inlier_translational_threshold)) & (np.abs(out["re"]) < np.float32(p.inlier_rotational_threshold))
        out["c"] = out["is_in"].sum(0)
    return out


def records_of(case, record_floats):
    """the relations' transforms as a closer call's records: T = words [0:16], column-major float; every word the validation must not read --
    the last row of T and everything behind it -- is NaN"""
    rec = np.full((case["n"], record_floats), np.nan, np.float32)
    rec[:, :16] = colmajor(case["tr"]).astype(np.float32)
    rec[:, [3, 7, 11, 15]] = np.nan
    return rec


def with_record_transforms(case):
    """the case whose tr are what a record carries: rounded to float, converted back"""
    c = dict(case)
    c["tr"] = case["tr"].astype(np.float32).astype(np.float64)
    c["name"] = case["name"] + "_f32"
    return c


def run_device(ctx, case, matrices=True, form="tr", place="host", counters=None, params=None, flags="case"):
    """pwn_hip_validate_relations -> the dict of run_host.  form: "tr" or a record size; place: "host", "device" or "mixed" (every other array on
    the device); flags: "case" or an array / None"""
    import ctypes as C
    from g2o_frontend_amd import api
    n = case["n"]
    fl = case["flags"] if isinstance(flags, str) else flags
    cnt = [np.ascontiguousarray(a, np.int32).copy() for a in (case["counters"] if counters is None else counters)]
    arrays = dict(tc=colmajor(case["tc"]), to=colmajor(case["to"]), tr=colmajor(case["tr"]) if form == "tr" else None,
                  records=None if form == "tr" else records_of(case, form), flags=None if fl is None else np.ascontiguousarray(fl, np.int32),
                  times_checked=cnt[0], cum_inlier=cnt[1], cum_outlier_times=cnt[2], decisions=np.full(n, -7, np.int32),
                  te=np.full((n, n), np.float32(-1)) if matrices else None, re=np.full((n, n), np.float32(-1)) if matrices else None)
    on_device = {}
    for k, (name, a) in enumerate(arrays.items()):
        if a is not None and (place == "device" or (place == "mixed" and k % 2 == 0)):
            on_device[name] = api.DeviceBuffer(ctx, a)
    arg = lambda name: C.c_void_p(on_device[name].data_ptr()) if name in on_device else vp(arrays[name])
    p = params_struct(case["params"] if params is None else params)
    rc = ctx._L.pwn_hip_validate_relations(ctx.h, C.byref(p), n, arg("tc"), arg("to"), arg("tr"), arg("records"), 0 if form == "tr" else form, arg("flags"),
                                           arg("times_checked"), arg("cum_inlier"), arg("cum_outlier_times"), arg("decisions"), arg("te"), arg("re"))
    got = {name: (on_device[name].numpy() if name in on_device else arrays[name]) for name in arrays}
    return dict(rc=rc, error=ctx._L.pwn_hip_last_error_string(ctx.h).decode() if rc else "", times_checked=got["times_checked"], cum_inlier=got["cum_inlier"],
                cum_outlier_times=got["cum_outlier_times"], decisions=got["decisions"], te=None if got["te"] is None else got["te"].T,
                re=None if got["re"] is None else got["re"].T)
