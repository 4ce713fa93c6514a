"""pwn_hip_track_pose_update -- the host compilation of what k_track_begin / k_track_end do between two alignments of a stream (csrc/pwn_track.h:
the guess, the pose chain, the re-orthonormalisation of every 50th frame, the key-cloud decision; pwn_tracker/pwn_tracker.cpp:132-185) -- against
the numpy arithmetic of api.PwnTracker.processFrame and against OracleTracker.processFrame driven with the same alignment result.  Every output
bit for bit.  No GPU.

The key-cloud decision.  The reference compares two floats (pwn_tracker.h:98, pwn_tracker.cpp:163-165); so does the library.  api.PwnTracker and
OracleTracker write `np.float32(fraction) < python_float`, which NumPy >= 2 evaluates in float32 (the Python scalar is weak) -- the reference's
rule -- and NumPy 1 evaluated in double.  The two rules differ only where the fraction EQUALS the float threshold and the float threshold lies
below its double (0.7, 0.35, 0.9: double says "switch", float says "keep"); for 0.66 and 0.4 the float lies above the double and both keep.  The
models below cast the threshold to float32 explicitly, so they state the reference's rule under either NumPy; the cases where a double comparison
would decide differently are counted and shown to exist."""
import numpy as np
import pytest

from oracle_tracker import OracleTracker

PIXELS = 120 * 160          # the "small" view


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _iso(rng, rot=0.2, trans=0.5, skew=0.0):
    """a float32 isometry near the identity; skew > 0 leaves the rotation block slightly non-orthonormal (what a chained float pose is)"""
    from g2o_frontend_amd import synth
    v = np.concatenate([rng.uniform(-trans, trans, 3), rng.uniform(-rot, rot, 3)])
    T = np.asarray(synth.v2t(v), np.float64)
    T[:3, :3] += rng.uniform(-skew, skew, (3, 3))
    T = T.astype(np.float32); T[3] = (0, 0, 0, 1)
    return T


def numpy_model(api, globalT, prevT, counter, keyframes, initialGuess, T, inliers, threshold):
    """api.PwnTracker.processFrame between `guess = ...` and `self._counter += 1`, with the alignment's result given"""
    guess = api.iso_mul(api.iso_mul(api.iso_inverse(prevT), globalT), initialGuess)
    G = api.iso_mul(prevT, T) if inliers > 0 else api.iso_mul(globalT, guess)
    if not (counter % 50):
        R = G[:3, :3].astype(np.float32)
        E = api._mul3(R.T, R); E[np.arange(3), np.arange(3)] -= np.float32(1)
        G[:3, :3] = (R - api._mul3(np.float32(0.5) * R, E)).astype(np.float32)
    G[3] = (0, 0, 0, 1)
    fraction = np.float32(inliers) / np.float32(PIXELS)
    new = bool(fraction < np.float32(threshold))
    return dict(globalT=G, previousCloudTransform=G.copy() if new else prevT.copy(), counter=counter + 1, numKeyframes=keyframes + int(new), newFrame=new,
                inliersFraction=fraction)


class _OracleWithResult:
    """the oracle's isometry arithmetic with a canned Aligner::align"""

    def __init__(self, O):
        self.O, self.result = O, None

    def iso_mul(self, A, B): return self.O.iso_mul(A, B)
    def iso_inverse(self, T): return self.O.iso_inverse(T)
    def reorthonormalize(self, T): return self.O.reorthonormalize(T)
    def aligner_params(self, *a, **k): return None
    def align(self, ap, ref, cur): return dict(self.result)


class _Tracker(OracleTracker):
    def makeCloud(self, K, off, depth):
        return "current", 120, 160, None


def oracle_model(O, globalT, prevT, counter, keyframes, T, inliers, threshold):
    proxy = _OracleWithResult(O)
    proxy.result = dict(T=T.copy(), inliers=int(inliers), error=0.0)
    otr = _Tracker(proxy, {}, {}, 2, float(np.float32(threshold)))
    otr.prev, otr.prevT, otr.globalT, otr.counter, otr.keyframes = "key", prevT.copy(), globalT.copy(), counter, keyframes
    out = otr.processFrame(None, np.eye(4, dtype=np.float32), None)
    return dict(globalT=otr.globalT, previousCloudTransform=otr.prevT, counter=otr.counter, numKeyframes=otr.keyframes, newFrame=out["newFrame"],
                switched=otr.prev == "current")


def cases():
    """(name, counter, inliers, threshold) x 24 each, every category the pose update branches on"""
    rng = np.random.default_rng(20240611)
    out = []
    n = 24
    for i in range(n):
        out.append(("inliers == 0", int(rng.integers(1, 200)), 0, 0.4))
        out.append(("inliers == 0 at counter % 50 == 0", 50 * int(rng.integers(0, 4)), 0, 0.4))
        for c in (49, 50, 51, 0, 1, 99, 100, 101):
            out.append(("counter %d" % c, c, int(rng.integers(1, PIXELS)), 0.4))
        k = int(rng.integers(2000, PIXELS - 2000))
        at = np.float32(k) / np.float32(PIXELS)
        out.append(("fraction at the threshold", int(rng.integers(1, 49)), k, float(at)))
        out.append(("fraction one float below the threshold", int(rng.integers(1, 49)), k, float(np.nextafter(at, np.float32(2)))))
        out.append(("fraction one float above the threshold", int(rng.integers(1, 49)), k, float(np.nextafter(at, np.float32(-1)))))
        for thr in (0.66, 0.4, 0.7, 0.35):       # thresholds whose float differs from their double, at equality and around it
            k0 = int(round(thr * PIXELS))
            assert np.float32(k0) / np.float32(PIXELS) == np.float32(thr)
            out.append(("threshold %.2f at equality" % thr, int(rng.integers(1, 49)), k0, thr))
            out.append(("threshold %.2f around equality" % thr, int(rng.integers(1, 49)), k0 + int(rng.choice([-2, -1, 1, 2])), thr))
    return out


def test_pose_update_matches_numpy_and_oracle_bit_for_bit(oracle):
    from g2o_frontend_amd import api
    rng = np.random.default_rng(7)
    I = np.eye(4, dtype=np.float32)
    seen, double_differs = {}, 0
    for name, counter, inliers, threshold in cases():
        globalT, prevT, T = _iso(rng, skew=1e-3), _iso(rng, skew=1e-3), _iso(rng, 0.05, 0.1)
        keyframes = int(rng.integers(1, 9))
        state = dict(globalT=globalT, previousCloudTransform=prevT, counter=counter, numKeyframes=keyframes, keySlot=3)
        new, res = api.track_pose_update(state, None, T, inliers, PIXELS, threshold, slot=5)
        m = numpy_model(api, globalT, prevT, counter, keyframes, I, T, inliers, threshold)
        o = oracle_model(oracle, globalT, prevT, counter, keyframes, T, inliers, threshold)
        for ref, who in ((m, "numpy"), (o, "oracle")):
            assert np.array_equal(_bits(new["globalT"]), _bits(ref["globalT"])), (name, who, counter, inliers)
            assert np.array_equal(_bits(new["previousCloudTransform"]), _bits(ref["previousCloudTransform"])), (name, who)
            assert (new["counter"], new["numKeyframes"], res["newFrame"]) == (ref["counter"], ref["numKeyframes"], ref["newFrame"]), (name, who, threshold, inliers)
        assert np.array_equal(_bits(res["globalT"]), _bits(new["globalT"]))
        assert _bits(np.float32(res["inliersFraction"])) == _bits(m["inliersFraction"]), name
        assert new["keySlot"] == (5 if res["newFrame"] else 3) and o["switched"] == res["newFrame"], name
        if "at the threshold" in name or "at equality" in name:
            assert not res["newFrame"], (name, threshold)           # equal is not below
        if "one float below" in name:
            assert res["newFrame"], name
        if "one float above" in name:
            assert not res["newFrame"], name
        double_differs += int(bool(float(m["inliersFraction"]) < float(threshold)) != res["newFrame"])
        seen[name] = seen.get(name, 0) + 1
    assert len(seen) >= 21 and min(seen.values()) >= 20, seen
    # the double comparison of NumPy 1 decides differently exactly at equality with 0.7 and 0.35, whose floats lie below their doubles
    assert double_differs == seen["threshold 0.70 at equality"] + seen["threshold 0.35 at equality"]


def test_pose_update_with_initial_guesses_matches_numpy_bit_for_bit():
    """the guess of pwn_tracker.cpp:132 with a caller's initial guess, in both branches of the pose chain"""
    from g2o_frontend_amd import api
    rng = np.random.default_rng(11)
    for i in range(200):
        globalT, prevT, T, guess = _iso(rng, skew=1e-3), _iso(rng, skew=1e-3), _iso(rng, 0.05, 0.1), _iso(rng, 0.1, 0.2)
        counter, inliers = int(rng.integers(0, 120)), (0 if i % 3 == 0 else int(rng.integers(1, PIXELS)))
        state = dict(globalT=globalT, previousCloudTransform=prevT, counter=counter, numKeyframes=2, keySlot=0)
        new, res = api.track_pose_update(state, guess, T, inliers, PIXELS, 0.5, slot=1)
        m = numpy_model(api, globalT, prevT, counter, 2, guess, T, inliers, 0.5)
        assert np.array_equal(_bits(new["globalT"]), _bits(m["globalT"])), i
        assert np.array_equal(_bits(new["previousCloudTransform"]), _bits(m["previousCloudTransform"])), i
        assert (new["counter"], new["numKeyframes"], res["newFrame"]) == (m["counter"], m["numKeyframes"], m["newFrame"]), i


def test_pose_update_results_are_rigid_after_the_correction():
    """a property, not a parity: the correction of every 50th frame pulls a drifted rotation back (R^T R - I shrinks)"""
    from g2o_frontend_amd import api
    rng = np.random.default_rng(3)
    for _ in range(20):
        prevT, T = _iso(rng, skew=2e-3), _iso(rng, 0.05, 0.1)
        state = dict(globalT=prevT, previousCloudTransform=prevT, counter=50, numKeyframes=1, keySlot=0)
        new, _ = api.track_pose_update(state, None, T, 1000, PIXELS, 0.0)
        plain, _ = api.track_pose_update(dict(state, counter=51), None, T, 1000, PIXELS, 0.0)
        err = lambda G: np.abs(G[:3, :3].astype(np.float64).T @ G[:3, :3].astype(np.float64) - np.eye(3)).max()
        assert err(new["globalT"]) < 0.5 * err(plain["globalT"])
        assert np.array_equal(new["globalT"][3], [0, 0, 0, 1])
