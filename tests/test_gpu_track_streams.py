"""pwn_hip_track_frames / api.PwnTrackerBatch: S depth streams tracked in lock-step, a run of F frames per stream in one submission
(PwnTracker::processFrame, pwn_tracker/pwn_tracker.cpp:106-215, with guess, pose chain, key-cloud decision and key switch on the device).

The yardstick is the single-stream tracker: api.PwnTracker, one per stream, frame by frame on the same frames (pwn_hip_convert_scaled +
pwn_hip_align per frame, bookkeeping on the host).  Everything is compared bit for bit: newFrame, inliers, error, T, globalT, numKeyframes, every
downloaded array of the final key cloud.  Frames are 240x320 uint16 renderings along synth.trajectory, tracked at scale 2: the 120x160 view
of the "small" configuration.

The streams (seed, metres and degrees per frame) were picked on the CPU with OracleTracker so that the key clouds switch where the tests need
them to (threshold 0.66; `*` = switch, the oracle's fractions, frame 0 is the first key):
  stream 0 (1, 0.06, 3.0)  * .695 *.616 .675 *.601 .690 *.629 .729 .671 *.625 .792 .738 .699 .665 *.639 .867 .804 .764
  stream 1 (2, 0.04, 2.0)  * .785 .746 .724 .711 .702 .687 .670 *.650 .736 .690 *.638 .721 .663 *.606 .705 *.656 .730
  stream 2 (6, 0.06, 3.0)  * .700 *.619 .726 *.646 .756 .683 *.612 .802 .733 .671 *.623 .853 .802 .762 .731 .712 .690
  stream 3 (4, 0.04, 2.0)  * .728 .676 *.640 .711 .670 *.638 .750 .712 .678 *.644 .772 .732 .696 .670 *.633 .765 .717
  stream 4 (5, 0.04, 2.0)  * .759 .715 .667 *.633 .776 .712 .663 *.624 .795 .742 .697 *.660 .851 .794 .747 .695 *.659
The conditions themselves are asserted on the single trackers' results, not on the code under test."""
import ctypes as C

import numpy as np
import pytest

from conftest import case_params
from oracle_tracker import OracleTracker

pytestmark = pytest.mark.gpu

ROWS, COLS, SCALE, THRESHOLD = 240, 320, 2, 0.66
STREAMS = [(1, 0.06, 3.0), (2, 0.04, 2.0), (6, 0.06, 3.0), (4, 0.04, 2.0), (5, 0.04, 2.0)]
NFRAMES = 18
KEYS = ("points", "normals", "curvature", "omega_p", "omega_n")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class World:
    """one context for the module: the frames of every stream, the collaborators, and the single-stream runs (computed once, shared)"""

    def __init__(self):
        from g2o_frontend_amd import api, synth
        from test_gpu_parity import gpu_objects
        self.api, self.synth = api, synth
        self.ctx = api.Context(0, ROWS, COLS, 32)
        _, self.converter, self.aligner = gpu_objects(self.ctx, "small")
        K2 = synth.scaled_K(synth.K_VGA, 2)
        self.K2 = K2
        self.Km = np.array([[K2[0], 0, K2[2]], [0, K2[1], K2[3]], [0, 0, 1]], np.float32)
        self.off = synth.v2t(np.array([0.0, 0.0, 0.0, 0.01, -0.005, 0.0])).astype(np.float32)
        self.raw, self.depth = [], []
        for seed, ts, rs in STREAMS:
            poses = synth.trajectory(seed, NFRAMES, ts, rs)
            self.raw.append([synth.render_depth_mm(seed, poses[k], ROWS, COLS, K2, hole_stream=k) for k in range(NFRAMES)])
            self.depth.append([self.ctx.DepthImage_convert_16UC1_to_32FC1(f) for f in self.raw[-1]])
        self._single = {}

    def single_tracker(self):
        tr = self.api.PwnTracker(self.aligner, self.converter); tr.setScale(SCALE); tr.setNewFrameInliersFraction(THRESHOLD)
        return tr

    def single(self, s, frames, off_key="off"):
        """api.PwnTracker over the frames (indices into the stream's list) -> (results, tracker); cached"""
        key = (s, tuple(frames), off_key)
        if key not in self._single:
            off = self.off if off_key == "off" else np.eye(4, dtype=np.float32)
            tr = self.single_tracker()
            self._single[key] = ([tr.processFrame(self.depth[s][k], off, self.Km) for k in frames], tr)
        return self._single[key]

    def batch(self, S, F):
        tb = self.api.PwnTrackerBatch(self.aligner, self.converter, S, F, ROWS, COLS, SCALE); tb.setNewFrameInliersFraction(THRESHOLD)
        return tb

    def close(self):
        self._single.clear()
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def same_result(g, r, where):
    """a frame's dict of the batch tracker against the single tracker's"""
    assert g["newFrame"] == r["newFrame"] and g["aligned"] == r["aligned"] and g["inliers"] == r["inliers"], (where, g["inliers"], r["inliers"])
    assert _bits(np.float32(g["error"])) == _bits(np.float32(r["error"])), where
    assert np.array_equal(_bits(g["globalT"]), _bits(r["globalT"])), where
    if r["aligned"]:
        assert np.array_equal(_bits(g["T"]), _bits(r["T"])), where
        assert _bits(np.float32(g["inliersFraction"])) == _bits(np.float32(r["inliersFraction"])), where
    else:
        assert g["T"] is None


def same_final(tb, s, tr, where):
    assert tb.numKeyframes(s) == tr.numKeyframes(), where
    assert np.array_equal(_bits(tb.globalT(s)), _bits(tr.globalT())), where
    st = tb.state(s)
    assert np.array_equal(_bits(st["previousCloudTransform"]), _bits(tr._previousCloudTransform)) and st["counter"] == tr._counter, where
    mine, ref = tb.keyCloud(s).arrays(), tr._previousCloud.arrays()
    for key in KEYS:
        assert mine[key].shape == ref[key].shape and np.array_equal(_bits(mine[key]), _bits(ref[key])), (where, key)


def schedule(S, F):
    """two calls of F frames; in the second call one stream idles in step 1 (F > 1).  -> per call the frame index per (step, stream), None = idle"""
    idle = 1 if S > 1 else 0
    calls, nxt = [], [0] * S
    for call in range(2):
        rows = []
        for f in range(F):
            row = []
            for s in range(S):
                if call == 1 and f == 1 and s == idle:
                    row.append(None); nxt[s] += 1                      # the frame is dropped: the stream's tracker never sees it
                else:
                    row.append(nxt[s]); nxt[s] += 1
            rows.append(row)
        calls.append(rows)
    return calls


def run_batch(world, tb, calls, off_key="off"):
    off = world.off if off_key == "off" else np.eye(4, dtype=np.float32)
    out = []
    for rows in calls:
        frames = [[None if k is None else world.raw[s][k] for s, k in enumerate(row)] for row in rows]
        out.append(tb.processFrames(frames, off, world.Km))
    return out


@pytest.mark.parametrize("S,F,off_key", [(S, F, "off") for S in (1, 3, 5) for F in (1, 4, 9)] + [(3, 4, "identity"), (5, 9, "identity")])
def test_equals_single_trackers(world, S, F, off_key):
    """one call of F frames (twice: from trackers without a key, then from trackers with one) against S api.PwnTracker runs, sub-batches of 2
    pairs (so the last sub-batch of a step is partial).  off_key: with the sensor offset every alignment projects its current cloud; with the identity it
    takes the cloud's own index image."""
    world.ctx.set_subbatch(2, 2)
    try:
        calls = schedule(S, F)
        tb = world.batch(S, F)
        got = run_batch(world, tb, calls, off_key)
        singles = []
        for s in range(S):
            seq = [row[s] for rows in calls for row in rows if row[s] is not None]
            singles.append(world.single(s, seq, off_key))
        pos = [0] * S
        switched_in_call = [[0] * S for _ in calls]
        mixed_step = False
        for c, rows in enumerate(calls):
            for f, row in enumerate(rows):
                news = []
                for s, k in enumerate(row):
                    if k is None:
                        assert got[c][f][s] is None
                        continue
                    r = singles[s][0][pos[s]]; pos[s] += 1
                    same_result(got[c][f][s], r, (S, F, c, f, s))
                    news.append(bool(r["newFrame"] and r["aligned"]))
                    switched_in_call[c][s] += int(news[-1])
                if 0 < f < F - 1 and any(news) and not all(news):
                    mixed_step = True
        for s in range(S):
            same_final(tb, s, singles[s][1], (S, F, s))
        # the conditions on the inputs, from the single trackers' runs
        if F > 1 and S > 1 and off_key == "off":
            assert mixed_step, "a stream switches its key in the middle of a call while another keeps its"
        if F == 9:
            assert max(max(row) for row in switched_in_call) >= 2, "a stream switches twice within one call"
    finally:
        world.ctx.set_subbatch(64, 64)


def test_seventeen_streams_take_the_batch_kernels(world):
    """17 streams in default sub-batches: a step's conversions run as one launch of the single-pass front end (16 frames and more) and its projections
    with four points per thread (8 pairs and more) -- still the single trackers' bits.  Stream s follows the frames of stream s % 5 from frame s // 5 on."""
    S, F = 17, 3
    tb = world.batch(S, F)
    first = lambda s: s // len(STREAMS)
    got = tb.processFrames([[world.raw[s % 5][first(s)] for s in range(S)]], world.off, world.Km)
    got += tb.processFrames([[world.raw[s % 5][first(s) + 1 + f] for s in range(S)] for f in range(F)], world.off, world.Km)
    switches = 0
    for s in range(S):
        ref, tr = world.single(s % 5, list(range(first(s), first(s) + 1 + F)))
        for f in range(1 + F):
            same_result(got[f][s], ref[f], (s, f))
            switches += int(ref[f]["newFrame"] and ref[f]["aligned"])
        same_final(tb, s, tr, s)
    assert switches >= 3


def test_chunking(world):
    """nine frames of three streams in one call, as 9 calls of 1, and as 4 + 5: the same bits in results and final state"""
    S, n = 3, 9
    runs = []
    for chunks in ([9], [1] * 9, [4, 5]):
        tb = world.batch(S, 9)
        res, k = [], 0
        for m in chunks:
            rows = [[world.raw[s][k + f] for s in range(S)] for f in range(m)]
            res += tb.processFrames(rows, world.off, world.Km); k += m
        runs.append((tb, res))
    tb0, res0 = runs[0]
    for tb, res in runs[1:]:
        for f in range(n):
            for s in range(S):
                same_result(res[f][s], res0[f][s], (f, s))
        for s in range(S):
            a, b = tb.state(s), tb0.state(s)
            assert np.array_equal(_bits(a["globalT"]), _bits(b["globalT"])) and np.array_equal(_bits(a["previousCloudTransform"]), _bits(b["previousCloudTransform"]))
            assert (a["counter"], a["numKeyframes"]) == (b["counter"], b["numKeyframes"]) == (n, sum(int(res0[f][s]["newFrame"]) for f in range(n)))
            x, y = tb.keyCloud(s).arrays(), tb0.keyCloud(s).arrays()
            for key in KEYS:
                assert np.array_equal(_bits(x[key]), _bits(y[key])), (s, key)


def test_against_the_oracle(world, oracle):
    """per stream: newFrame equal in every frame, |inliers diff| <= 4, |globalT diff| < 5e-5 -- the bars test_tracker.py holds the single tracker to"""
    S, n = 3, 9
    _, _, _, conv, alig = case_params("small")
    tb = world.batch(S, n)
    got = tb.processFrames([[world.raw[s][f] for s in range(S)] for f in range(n)], world.off, world.Km)
    worst_inl, worst_pose = 0, 0.0
    for s in range(S):
        otr = OracleTracker(oracle, conv, alig, SCALE, THRESHOLD)
        for f in range(n):
            o = otr.processFrame(oracle.convert_16u_to_32f(world.raw[s][f]), world.off, world.Km)
            g = got[f][s]
            if f > 0:
                worst_inl = max(worst_inl, abs(g["inliers"] - o["inliers"]))
            worst_pose = max(worst_pose, float(np.abs(g["globalT"] - o["globalT"]).max()))
            assert g["newFrame"] == o["newFrame"], (s, f, g["inliers"], o.get("inliers"))
        assert tb.numKeyframes(s) == otr.keyframes
    print(f"track_streams vs oracle: worst |inliers diff| {worst_inl}, worst |globalT diff| {worst_pose:.2e}")
    assert worst_inl <= 4 and worst_pose < 5e-5, (worst_inl, worst_pose)


def test_reorthonormalisation_and_zero_inliers(world):
    """counter = 49 on both sides, then three frames (counters 49, 50, 51: the correction of pwn_tracker.cpp:154-159 in the second); stream 1 gets an
    all-zero frame in the second step and stream 2 in the first: an empty cloud, no inliers, _globalT = _globalT * guess (:150) and a key cloud
    without points behind it."""
    S = 3
    zero = np.zeros((ROWS, COLS), np.uint16)
    zerof = world.ctx.DepthImage_convert_16UC1_to_32FC1(zero)
    tb = world.batch(S, 3)
    first = tb.processFrames([[world.raw[s][f] for s in range(S)] for f in range(2)], world.off, world.Km)
    for s in range(S):
        tb.setState(s, counter=49)
    rows = [[world.raw[s][2 + f] for s in range(S)] for f in range(3)]
    rows[1][1] = zero; rows[0][2] = zero
    got = tb.processFrames(rows, world.off, world.Km)
    saw_zero = 0
    for s in range(S):
        tr = world.single_tracker()
        for f in range(2):
            same_result(first[f][s], tr.processFrame(world.depth[s][f], world.off, world.Km), (s, f))
        tr._counter = 49
        for f in range(3):
            d = zerof if rows[f][s] is zero else world.depth[s][2 + f]
            r = tr.processFrame(d, world.off, world.Km)
            same_result(got[f][s], r, (s, f))
            saw_zero += int(r["aligned"] and r["inliers"] == 0)
        assert tb.state(s)["counter"] == tr._counter == 52
        assert tb.numKeyframes(s) == tr.numKeyframes() and np.array_equal(_bits(tb.globalT(s)), _bits(tr.globalT()))
    assert saw_zero >= 2, "the single tracker reports inliers == 0 on the empty frames"
    # a key cloud may be empty: after an all-zero last frame the state still goes through get_state / set_state
    last = tb.processFrames([[zero if s == 0 else world.raw[s][5] for s in range(S)]], world.off, world.Km)
    assert last[0][0]["newFrame"] and tb.keyCloud(0).size() == 0
    before = bytes(tb.states())
    tb.setState(0, counter=tb.state(0)["counter"])
    assert bytes(tb.states()) == before


def _fallbacks(ctx):
    n = C.c_int(0)
    ctx.check(ctx._L.pwn_hip_debug_projection_fallbacks(ctx.h, C.byref(n)))
    return n.value


def test_give_up_repeat(world):
    """settle guard at 0 rounds: every collision of a projection gives up, the call is made again with the two-pass projection from the states it
    started with -- results, states, slots and key clouds are those of clean calls"""
    S, F = 3, 4
    calls = schedule(S, F)
    clean = world.batch(S, F)
    want = run_batch(world, clean, calls)
    hooked = world.batch(S, F)
    world.ctx.check(world.ctx._L.pwn_hip_debug_set_settle_guard(world.ctx.h, 0))
    try:
        before = _fallbacks(world.ctx)
        got = run_batch(world, hooked, calls)
        assert _fallbacks(world.ctx) == before + len(calls)
    finally:
        world.ctx.check(world.ctx._L.pwn_hip_debug_set_settle_guard(world.ctx.h, -1))
    for c, rows in enumerate(calls):
        for f, row in enumerate(rows):
            for s, k in enumerate(row):
                if k is None:
                    assert got[c][f][s] is None
                else:
                    same_result(got[c][f][s], want[c][f][s], (c, f, s))
    assert bytes(hooked.states()) == bytes(clean.states())
    for s in range(S):
        x, y = hooked.keyCloud(s).arrays(), clean.keyCloud(s).arrays()
        for key in KEYS:
            assert np.array_equal(_bits(x[key]), _bits(y[key])), (s, key)


def test_refusals_touch_nothing(world):
    api = world.api
    S, F = 3, 4
    tb = world.batch(S, F)
    tb.processFrames([[world.raw[s][f] for s in range(S)] for f in range(2)], world.off, world.Km)
    L, ctx = world.ctx._L, world.ctx
    cp, ap = tb.callParams(world.off, world.Km)
    frames = [world.raw[s][2 + f] for f in range(F) for s in range(S)]
    ptrs = (C.c_void_p * (F * S))(*[api._ptr(d) for d in frames])
    res = (api.TrackResult * (F * S))()
    C.memset(res, 0x5A, C.sizeof(res))

    def snapshot():
        return bytes(tb.states()), [{k: v.copy() for k, v in tb.keyCloud(s).arrays().items()} for s in range(S)], bytes(res)

    def call(ctx_h=ctx.h, tr=tb.h, cpp=C.byref(cp), app=C.byref(ap), nF=F, fr=ptrs, out=res):
        return L.pwn_hip_track_frames(ctx_h, tr, cpp, app, nF, fr, 0.001, 0.01, None, THRESHOLD, out)

    before = snapshot()
    bad_size = api.AlignerParams.from_buffer_copy(ap); bad_size.rows = ap.rows + 1
    too_many = api.AlignerParams.from_buffer_copy(ap); too_many.outer_iterations = 100
    other = api.Context(0, ROWS, COLS, 2)
    try:
        small_ctx_tracker = C.c_void_p()
        assert L.pwn_hip_tracker_create(other.h, 3, F, ROWS, COLS, SCALE, C.byref(small_ctx_tracker)) == 6      # S above the context's max_batch
        assert not small_ctx_tracker.value
        refused = [call(ctx_h=None), call(tr=None), call(cpp=None), call(app=None), call(fr=None), call(out=None), call(nF=0), call(nF=F + 1),
                   call(app=C.byref(bad_size)), call(app=C.byref(too_many)), call(ctx_h=other.h)]
    finally:
        other.close()
    assert all(rc in (1, 6) for rc in refused), refused
    after = snapshot()
    assert after[0] == before[0] and after[2] == before[2]
    for a, b in zip(after[1], before[1]):
        for key in KEYS:
            assert np.array_equal(_bits(a[key]), _bits(b[key])), key
    # set_state: a key slot that holds no cloud, a slot outside the ring
    st = tb.states()
    bad = api.TrackerState.from_buffer_copy(st[0]); bad.key_slot = F + 1
    assert L.pwn_hip_tracker_set_state(tb.h, 0, 1, C.byref(bad)) == 1
    bad.key_slot = F                                     # two frames so far: slots 0 and 1 hold clouds, the last one none
    assert L.pwn_hip_tracker_set_state(tb.h, 0, 1, C.byref(bad)) == 1
    assert bytes(tb.states()) == before[0]
    # and the tracker still tracks: the refused calls left nothing behind
    ok = tb.processFrames([[world.raw[s][2 + f] for s in range(S)] for f in range(2)], world.off, world.Km)
    for s in range(S):
        ref, _ = world.single(s, list(range(4)))
        for f in range(2):
            same_result(ok[f][s], ref[2 + f], (s, f))
    # init(): PwnTracker::init -- the next frame is a first frame again
    tb.init()
    again = tb.processFrames([[world.raw[s][0] for s in range(S)]], world.off, world.Km)
    assert all(r["newFrame"] and not r["aligned"] for r in again[0]) and all(tb.numKeyframes(s) == 1 for s in range(S))


def _host_waits(ctx):
    n = C.c_int(0)
    ctx.check(ctx._L.pwn_hip_debug_host_waits(ctx.h, C.byref(n)))
    return n.value


def test_initial_guesses(world):
    """a non-identity initial guess per (frame, stream) -- guess = previousCloudTransform^-1 * globalT * initialGuess (pwn_tracker.cpp:132) on the device --
    against api.PwnTracker.processFrame(initialGuess=...), bit for bit; one entry is None (identity)"""
    S, F = 3, 4
    rng = np.random.default_rng(5)
    def guess():
        v = np.concatenate([rng.uniform(-0.01, 0.01, 3), rng.uniform(-0.004, 0.004, 3)])
        return world.synth.v2t(v).astype(np.float32)
    guesses = [[guess() for s in range(S)] for f in range(1 + F)]
    guesses[2][1] = None
    tb = world.batch(S, F)
    got = tb.processFrames([[world.raw[s][0] for s in range(S)]], world.off, world.Km, guesses=[guesses[0]])
    got += tb.processFrames([[world.raw[s][1 + f] for s in range(S)] for f in range(F)], world.off, world.Km, guesses=guesses[1:])
    differs = 0
    for s in range(S):
        tr = world.single_tracker()
        plain, _ = world.single(s, list(range(1 + F)))
        for f in range(1 + F):
            r = tr.processFrame(world.depth[s][f], world.off, world.Km, initialGuess=guesses[f][s])
            same_result(got[f][s], r, (s, f))
            differs += int(f > 0 and not np.array_equal(_bits(r["globalT"]), _bits(plain[f]["globalT"])))
        same_final(tb, s, tr, s)
    assert differs >= S, "the guesses change the single trackers' poses, so the test would see a guess that is dropped or misplaced"


def test_launch_shape(world):
    """one call of F = 4, S = 5 with profiling on: one host wait, k_track_begin and k_track_end once per step, every reference projection made (the
    reference's own index image is never taken: the host does not know the guess)"""
    S, F = 5, 4
    ctx = world.ctx
    tb = world.batch(S, F)
    tb.processFrames([[world.raw[s][0] for s in range(S)]], world.off, world.Km)
    ctx.set_profiling(True)
    try:
        waits = _host_waits(ctx)
        tb.processFramesRaw([[world.raw[s][1 + f] for s in range(S)] for f in range(F)], world.off, world.Km)
        waits = _host_waits(ctx) - waits
        launches = {s: ctx.stage_ms(s)[1] for s in ("track_begin", "track_end", "project_ref", "project_cur", "corr_linearize", "solve")}
    finally:
        ctx.set_profiling(False)
    outer = world.aligner.outerIterations()
    assert waits == 1, waits          # every wait of the library for one of the context's streams is counted (pwn_hip_debug_host_waits)
    assert launches["track_begin"] == F and launches["track_end"] == F, launches
    assert launches["project_ref"] == F * outer and launches["project_cur"] == F, launches      # S = 5 pairs: one sub-batch per step
    assert launches["solve"] == launches["corr_linearize"] == F * outer * world.aligner.innerIterations(), launches
