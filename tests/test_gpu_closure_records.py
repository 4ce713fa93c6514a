"""Closure records: pwn_hip_closure_batch_records (include/pwn_hip.h) -- the match record plus Aligner::omega() and the rest of
Aligner::_computeStatistics, whose 6x6 math runs on the device (k_pair_statistics) with the bits of the host's pwn_hip_compute_statistics.

Comparison rule everywhere (statistics_systems.words_equal): bit equality per word; two NaNs are equal whatever their sign and payload; a NaN
on one side only, or an infinity of the other sign, is a difference."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import early_stop as E
import statistics_systems as S
from conftest import case_params, make_depth_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 128
KINDS = ("identity", "odometry", "far")


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cm(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).reshape(4, 4).T.reshape(-1))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stat_words(st):
    """[n, 47] float32 of an AlignStatistics array in the record's order: omega, mean, both ratios, error, inliers, computed"""
    out = np.zeros((len(st), 47), np.float32)
    for i, q in enumerate(st):
        out[i, :36] = np.frombuffer(q.omega, np.float32); out[i, 36:42] = np.frombuffer(q.mean, np.float32)
        out[i, 42] = np.float32(q.translational_eigen_ratio); out[i, 43] = np.float32(q.rotational_eigen_ratio)
        out[i, 44] = np.float32(q.error); out[i, 45] = np.float32(q.inliers); out[i, 46] = 1.0
    return out


def _same(a, b, what):
    eq = S.words_equal(np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1))
    assert eq.all(), (what, np.where(~eq)[0][:8], np.asarray(a, np.float32).reshape(-1)[~eq][:4], np.asarray(b, np.float32).reshape(-1)[~eq][:4])


class Rig:
    def __init__(self, name, seeds, max_batch, omega_storage="sym6"):
        from g2o_frontend_amd import api
        from test_gpu_parity import gpu_objects
        self.name = name
        self.rows, self.cols, self.K, _, _ = case_params(name)
        self.ctx = api.Context(0, self.rows, self.cols, max_batch, omega_storage=omega_storage)
        _, self.converter, self.aligner = gpu_objects(self.ctx, name)
        self.refs, self.curs, self.raw = [], [], []
        for s in seeds:
            ref, cur, _, ref_mm, cur_mm = make_depth_pair(name, s)
            r, c = api.Cloud(self.ctx, self.rows * self.cols), api.Cloud(self.ctx, self.rows * self.cols)
            self.converter.compute(r, ref, images=False); self.converter.compute(c, cur, images=False)
            self.refs.append(r); self.curs.append(c); self.raw.append((ref_mm, cur_mm))
        self.guesses = [E.guess_for(s, KINDS[i % 3]) for i, s in enumerate(seeds)]

    def args(self, idx):
        n = len(idx)
        return (n, (C.c_void_p * n)(*[self.refs[i].h for i in idx]), (C.c_void_p * n)(*[self.curs[i].h for i in idx]),
                np.stack([_cm(self.guesses[i]) for i in idx]))

    def closure(self, idx, device=False, ids=None, first=0, results=True, statistics=True, fill=-7.0):
        """pwn_hip_closure_batch_records -> dict(rec [n, 128], res, sc, st)"""
        from g2o_frontend_amd import api
        from g2o_frontend_amd._lib import AlignStatistics, MatchResult
        ctx, p = self.ctx, self.aligner.params()
        n, refs, curs, g = self.args(idx)
        res = (api.AlignResult * n)() if results else None; sc = (MatchResult * n)() if results else None
        st = (AlignStatistics * n)() if statistics else None
        host = np.full((n, R), fill, np.float32)
        dev = ctx.upload(host) if device else None
        ctx.check(ctx._L.pwn_hip_closure_batch_records(ctx.h, C.byref(p), n, refs, curs, _vp(g), 50.0, _vp(ids), first, res, sc, st,
                                                       C.c_void_p(dev.data_ptr()) if device else _vp(host)))
        out = dict(rec=dev.numpy().reshape(n, R) if device else host, st=st)
        if results:
            r = np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=n).copy(); r["total_time_ms"] = 0
            out["res"] = r; out["sc"] = np.frombuffer(sc, np.uint8).reshape(n, -1).copy()
        return out

    def existing(self, idx, ids=None, first=0):
        """the calls the closure record is made of: pwn_hip_match_batch_records, pwn_hip_align_batch_ex, pwn_hip_match_batch"""
        from g2o_frontend_amd import api
        from g2o_frontend_amd._lib import AlignStatistics, MatchResult
        ctx, L, p = self.ctx, self.ctx._L, self.aligner.params()
        n, refs, curs, g = self.args(idx)
        rec72 = np.full((n, api.MATCH_RECORD_FLOATS), -7.0, np.float32)
        ctx.check(L.pwn_hip_match_batch_records(ctx.h, C.byref(p), n, refs, curs, _vp(g), 50.0, _vp(ids), first, None, None, _vp(rec72)))
        res = (api.AlignResult * n)(); sc = (MatchResult * n)(); st = (AlignStatistics * n)()
        ctx.check(L.pwn_hip_align_batch_ex(ctx.h, C.byref(p), n, refs, curs, _vp(g), res, 50.0, sc, st))
        res2 = (api.AlignResult * n)(); sc2 = (MatchResult * n)()
        ctx.check(L.pwn_hip_match_batch(ctx.h, C.byref(p), n, refs, curs, _vp(g), 50.0, res2, sc2))
        r = np.frombuffer(res2, dtype=api.ALIGN_RESULT_DTYPE, count=n).copy(); r["total_time_ms"] = 0
        rex = np.frombuffer(res, dtype=api.ALIGN_RESULT_DTYPE, count=n).copy()
        return dict(rec72=rec72, st=st, T=rex["T"].copy(), res=r, sc=np.frombuffer(sc2, np.uint8).reshape(n, -1).copy())

    def close(self):
        self.ctx.close()


def check(oracle, got, want, n, computed=True):
    """a closure call's outputs against the existing calls' for the same pairs (and against the oracle's statistics of the GPU's H and T)"""
    rec = got["rec"]
    assert np.array_equal(_bits(rec[:, :72]), _bits(want["rec72"]))
    assert not np.any(_bits(rec[:, 119:]))
    ex = _stat_words(want["st"])
    if computed:
        _same(rec[:, 72:119], ex, "record against pwn_hip_align_batch_ex")
        assert (rec[:, 118] == 1.0).all()
        for i in range(n):
            q = want["st"][i]
            H = np.frombuffer(q.H, np.float32).reshape(6, 6).T; T = want["T"][i].reshape(4, 4).T
            _same(rec[i, 72:116], S.oracle_words(oracle, H, T), ("record against the oracle", i))
    else:
        assert not np.any(_bits(rec[:, 72:119]))
    if got.get("st") is not None:
        _same(_stat_words(got["st"])[:, :46], rec[:, 72:118], "host statistics against the record")
        for a, b in zip(got["st"], want["st"]):
            assert bytes(a.H) == bytes(b.H) and bytes(a.b) == bytes(b.b)
    if "res" in got:
        assert got["res"].tobytes() == want["res"].tobytes() and got["sc"].tobytes() == want["sc"].tobytes()


@pytest.fixture(scope="module")
def small():
    rig = Rig("small", tuple(range(9)), 16)
    yield rig
    rig.close()


# ------------------------------------------------------------------------------------------------------------ the kernel on injected systems
def test_hook_on_injected_systems_of_every_family(oracle):
    """k_pair_statistics as shipped on every family of tests/statistics_systems.py, 1 ... 129 systems per launch through a context made for 4
    pairs (its pair arrays grow), against oracle.compute_statistics.  The symbol does not exist before this feature."""
    from g2o_frontend_amd import api
    ctx = api.Context(0, 120, 160, 4)
    try:
        classes = {}
        for fam in S.FAMILIES:
            H, T = S.systems(fam, 129)
            want = np.stack([S.oracle_words(oracle, H[i], T[i]) for i in range(129)])
            Hc = np.ascontiguousarray(H.transpose(0, 2, 1).reshape(129, 36)); Tc = np.ascontiguousarray(T.transpose(0, 2, 1).reshape(129, 16))
            for n in (129, 1, 2, 63, 64, 65):
                out = np.full((n, 44), -7.0, np.float32)
                ctx.check(ctx._L.pwn_hip_debug_statistics_eval(ctx.h, n, _vp(Hc), _vp(Tc), _vp(out)))
                eq = S.words_equal(out.reshape(-1), want[:n].reshape(-1)).reshape(n, 44)
                assert eq.all(), (fam, n, np.argwhere(~eq)[:6], out[~eq][:4], want[:n][~eq][:4])
            classes[fam] = {c: [S.outcome(w) for w in want].count(c) for c in ("finite", "nonfinite", "zero")}
        print(classes)
        assert sum(c["finite"] for c in classes.values()) >= 0.4 * 129 * len(classes)
        # bad arguments are status codes
        assert ctx._L.pwn_hip_debug_statistics_eval(ctx.h, 1, None, _vp(Tc), _vp(out)) == 1
        assert ctx._L.pwn_hip_debug_statistics_eval(ctx.h, -1, _vp(Hc), _vp(Tc), _vp(out)) == 1
        assert ctx._L.pwn_hip_debug_statistics_eval(ctx.h, 0, None, None, None) == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------ the records
@pytest.mark.parametrize("n", [1, 5, 9])
def test_records_carry_match_record_and_statistics(oracle, small, n):
    idx = list(range(n))
    ids = np.arange(300, 300 + n, dtype=np.int32)[::-1].copy()
    want = small.existing(idx, first=11); want_ids = small.existing(idx, ids=ids)
    for sub, streams in ((64, 4), (2, 2)):                      # the default plan; sub-batches of 2 on two streams
        small.ctx.set_subbatch(64, sub); small.ctx.set_concurrency(streams)
        try:
            host = small.closure(idx, device=False, first=11)
            dev = small.closure(idx, device=True, first=11, results=False, statistics=False)
            with_ids = small.closure(idx, device=True, ids=ids)
        finally:
            small.ctx.set_subbatch(64, 64); small.ctx.set_concurrency(4)
        check(oracle, host, want, n)
        assert np.array_equal(_bits(dev["rec"]), _bits(host["rec"]))
        check(oracle, with_ids, want_ids, n)
        assert np.array_equal(with_ids["rec"][:, 19], ids.astype(np.float32)) and np.array_equal(host["rec"][:, 19], np.arange(11, 11 + n, dtype=np.float32))
    assert np.all(np.isfinite(host["rec"][:, 72:119])) and np.all(host["rec"][:, 72] > 0)        # real alignments: a regular omega


def test_one_vga_pair(oracle):
    """one 480 x 640 pair: the 150-workgroup latency shape of the linearize pass in front of the kernel"""
    rig = Rig("vga", (0,), 1)
    try:
        want = rig.existing([0], first=3)
        check(oracle, rig.closure([0], first=3), want, 1)
        assert np.array_equal(_bits(rig.closure([0], device=True, first=3, results=False, statistics=False)["rec"]), _bits(rig.closure([0], first=3)["rec"]))
    finally:
        rig.close()


def test_no_outer_iterations_leave_the_statistics_words_zero(oracle, small):
    idx = [0, 1, 2]
    small.aligner.setOuterIterations(0)
    try:
        want = small.existing(idx)
        for device in (False, True):
            got = small.closure(idx, device=device)
            check(oracle, got, want, 3, computed=False)
            assert (got["rec"][:, 118] == 0).all() and (got["rec"][:, 18] == 0).all()
            assert not np.any(np.frombuffer(got["st"], np.uint8))              # as fill_statistics(nullptr) leaves them
    finally:
        small.aligner.setOuterIterations(E.OUTER)


def test_early_stop_gives_the_statistics_of_pwn_hip_align_batch_ex(oracle, small):
    idx = list(range(6))
    small.ctx.set_convergence(*E.LOOSE)
    try:
        want = small.existing(idx)
        got = small.closure(idx)
        steps = small.aligner.lastSteps(0, 6)
    finally:
        small.ctx.clear_convergence()
    assert sum(1 for s in steps if s["converged"]) >= 2 and len({s["iterations"] for s in steps}) >= 2, steps
    check(oracle, got, want, 6)
    assert sorted(set(got["rec"][:, 18])) == sorted({float(s["iterations"]) for s in steps})


def test_forced_two_pass_repeat_gives_the_same_bits(oracle, small):
    idx = list(range(5))
    ctx, L = small.ctx, small.ctx._L
    want = small.closure(idx, device=True)
    n0 = C.c_int(0); n1 = C.c_int(0)
    ctx.check(L.pwn_hip_debug_projection_fallbacks(ctx.h, C.byref(n0)))
    ctx.check(L.pwn_hip_debug_set_settle_guard(ctx.h, 0))
    try:
        got = small.closure(idx, device=True)
    finally:
        ctx.check(L.pwn_hip_debug_set_settle_guard(ctx.h, 4096))
    ctx.check(L.pwn_hip_debug_projection_fallbacks(ctx.h, C.byref(n1)))
    assert n1.value - n0.value == 1
    assert np.array_equal(_bits(got["rec"]), _bits(want["rec"])) and (got["rec"][:, 63] == 0).all()
    assert got["res"].tobytes() == want["res"].tobytes() and got["sc"].tobytes() == want["sc"].tobytes()
    assert bytes(got["st"]) == bytes(want["st"])


def test_refusals_touch_nothing(small):
    from g2o_frontend_amd import api
    from g2o_frontend_amd._lib import AlignStatistics
    from test_gpu_scaled_batch import flat_bytes
    ctx, L, p = small.ctx, small.ctx._L, small.aligner.params()
    n, refs, curs, g = small.args([0, 1])
    before = [flat_bytes(c).tobytes() for c in (small.refs[0], small.curs[0], small.refs[1], small.curs[1])]
    rec = np.full((2, R), -7.0, np.float32)
    st = (AlignStatistics * 2)()
    # a null `records`
    assert L.pwn_hip_closure_batch_records(ctx.h, C.byref(p), n, refs, curs, _vp(g), 50.0, None, 0, None, None, st, None) == 1
    # current clouds of mixed omega storages
    ctx.set_omega_storage("exact9")
    try:
        odd = api.Cloud(ctx, small.rows * small.cols)
        small.converter.compute(odd, make_depth_pair("small", 1)[1], images=False)
    finally:
        ctx.set_omega_storage("sym6")
    mixed = (C.c_void_p * 2)(small.curs[0].h, odd.h)
    odd_before = flat_bytes(odd).tobytes()
    assert L.pwn_hip_closure_batch_records(ctx.h, C.byref(p), n, refs, mixed, _vp(g), 50.0, None, 0, None, None, st, _vp(rec)) == 1
    assert flat_bytes(odd).tobytes() == odd_before
    # a cloud above 2^21 points
    big = api.Cloud(ctx, (1 << 21) + 2 * small.rows * small.cols)
    I = np.eye(4, dtype=np.float32)
    while big.size() <= (1 << 21):
        big.add(small.refs[0], I)
    size = big.size()
    huge = (C.c_void_p * 2)(small.refs[0].h, big.h)
    assert L.pwn_hip_closure_batch_records(ctx.h, C.byref(p), n, huge, curs, _vp(g), 50.0, None, 0, None, None, st, _vp(rec)) == 6
    assert big.size() == size
    assert (rec == -7.0).all() and not np.any(np.frombuffer(st, np.uint8))
    assert before == [flat_bytes(c).tobytes() for c in (small.refs[0], small.curs[0], small.refs[1], small.curs[1])]
    dev = ctx.upload(rec)
    assert L.pwn_hip_closure_batch_records(ctx.h, C.byref(p), n, huge, curs, _vp(g), 50.0, None, 0, None, None, None, C.c_void_p(dev.data_ptr())) == 6
    assert (dev.numpy() == -7.0).all()


def test_python_mirror_and_cpp_mirror(tmp_path):
    """PwnMatcherBase.matchCloudsBatchClosureRecords, the relation dicts of shard.unpack_closure_records and api's result builder against the
    record; tools/pwn_hip_closure_records_check (the C++ mirror) reproduces the Python mirror's bytes from the same frames."""
    from g2o_frontend_amd import api, build, shard
    from test_gpu_parity import gpu_objects
    build.build_tools()
    rows, cols, K, _, _ = case_params("small")
    seeds = (0, 1, 2, 3)
    n = len(seeds)
    ctx = api.Context(0, rows, cols, 8)
    try:
        _, converter, aligner = gpu_objects(ctx, "small")
        matcher = api.PwnMatcherBase(aligner, converter); matcher.setScale(1)
        raw = [make_depth_pair("small", s)[3:5] for s in seeds]
        refs = [api.Cloud(ctx, rows * cols) for _ in range(n)]; curs = [api.Cloud(ctx, rows * cols) for _ in range(n)]
        converter.computeBatch(refs + curs, [r for r, _ in raw] + [c for _, c in raw], raw_scale=0.001)
        guesses = [E.guess_for(s, KINDS[i % 3]) for i, s in enumerate(seeds)]
        Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float32); I = np.eye(4, dtype=np.float32)
        rec = np.full((n, api.CLOSURE_RECORD_FLOATS), -7.0, np.float32)
        res, sc, st = matcher.matchCloudsBatchClosureRecords(refs, curs, I, I, Km, rows, cols, rec, guesses, first_pair_id=40, want_statistics=True)
        dev = ctx.upload(np.full((n, api.CLOSURE_RECORD_FLOATS), -3.0, np.float32))
        assert matcher.matchCloudsBatchClosureRecords(refs, curs, I, I, Km, rows, cols, dev, guesses, first_pair_id=40, want_results=False) is None
        assert np.array_equal(_bits(dev.numpy().reshape(n, -1)), _bits(rec))
        base = matcher.matchCloudsBatch(refs, curs, I, I, Km, rows, cols, guesses)
        with pytest.raises(ValueError):
            matcher.matchCloudsBatchClosureRecords(refs, curs, I, I, Km, rows, cols, np.zeros((n, api.MATCH_RECORD_FLOATS), np.float32), guesses)
    finally:
        ctx.close()
    assert api.CLOSURE_RECORD_FLOATS == shard.CLOSURE_RECORD_FLOATS == R
    rel = shard.unpack_closure_records(rec)
    for i in range(n):
        q, d, b = rec[i], rel[i], base[i]
        m = api.PwnMatcherBase.closureResult(q)
        omega = q[72:108].reshape(6, 6).T.astype(np.float64)
        for r in (d, m):
            assert r["informationMatrix"].dtype == np.float64 and np.array_equal(r["informationMatrix"], omega)
            assert np.array_equal(r["transform"], b["transform"]) and r["transform"].dtype == np.float64
            assert (r["image_nonZeros"], r["image_outliers"], r["image_inliers"]) == (b["image_nonZeros"], b["image_outliers"], b["image_inliers"])
            assert np.float32(r["image_reprojectionDistance"]).view(np.uint32) == np.float32(b["image_reprojectionDistance"]).view(np.uint32)
            assert r["cloud_inliers"] == b["cloud_inliers"]
            assert np.float32(r["translationalEigenRatio"]) == q[114] and np.float32(r["rotationalEigenRatio"]) == q[115] and r["statisticsComputed"]
        assert d["pair_id"] == 40 + i
        assert d["solutionValid"] == (not (q[115] > 50.0 or q[114] > 50.0))
        assert np.array_equal(np.frombuffer(st[i].omega, np.float32), q[72:108])
        assert np.array_equal(b["informationMatrix"], np.eye(6) * 100.0)          # v1's matrix stays where it was
        assert np.allclose(omega, omega.T, rtol=1e-3, atol=1e-3 * np.abs(omega).max()) and np.all(np.linalg.eigvalsh((omega + omega.T) / 2) > 0)
    assert not shard.unpack_closure_records(np.zeros((1, R), np.float32))[0]["statisticsComputed"]
    path = os.path.join(str(tmp_path), "closure_records.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<6i4f", n, rows, cols, E.OUTER, 1, 40, *[float(np.float32(k)) for k in K]))
        for r, c in raw:
            f.write(np.ascontiguousarray(r, np.uint16).tobytes()); f.write(np.ascontiguousarray(c, np.uint16).tobytes())
        for T in guesses:
            f.write(_cm(T).tobytes())
        f.write(rec.tobytes())
    exe = os.path.join(ROOT, "tools", "pwn_hip_closure_records_check")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 differences" in r.stdout and f"{n} with statistics" in r.stdout
    # the tool finds a changed word
    bad = rec.copy(); bad[1, 80] = np.nextafter(bad[1, 80], np.float32(np.inf))
    with open(path, "r+b") as f:
        f.seek(-rec.nbytes, 2); f.write(bad.tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout + r.stderr
