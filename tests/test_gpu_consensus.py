"""The consensus validation of closures on the device (pwn_hip_validate_relations) against the host call (pwn_hip_validate_relations_host), which
expands the same text: both error matrices as uint32, the three counters and the decisions are equal in every case of tests/consensus_cases.py,
so a difference is a bug, not a tolerance.  Also: the closed form of the cluster case at sizes the host is not run at, every input form,
accumulation over calls, the errors, the batch calls next to it, and the Python mirror."""
import ctypes as C

import numpy as np
import pytest

import consensus_cases as cc

pytestmark = pytest.mark.gpu

COUNTERS = ("times_checked", "cum_inlier", "cum_outlier_times", "decisions")
_HOST = {}


@pytest.fixture(scope="module")
def ctx():
    from g2o_frontend_amd import api
    c = api.Context(device=0, max_rows=120, max_cols=160, max_batch=2)
    yield c
    c.close()


def host(case, **kw):
    key = (case["name"], tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _HOST:
        _HOST[key] = cc.run_host(case, **kw)
    return _HOST[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_equal(d, h, name, matrices=True):
    assert d["rc"] == h["rc"] == 0, (name, d["rc"], d.get("error"), h["rc"])
    for k in COUNTERS:
        assert np.array_equal(d[k], h[k]), (name, k)
    if matrices:
        for k in ("te", "re"):
            assert np.array_equal(bits(d[k]), bits(h[k])), (name, k, int((bits(d[k]) != bits(h[k])).sum()))


def test_device_equals_host_bit_for_bit(ctx):
    for case in cc.all_cases():
        h = host(case)
        assert_equal(cc.run_device(ctx, case), h, case["name"])
        assert_equal(cc.run_device(ctx, case, matrices=False), h, case["name"], matrices=False)      # the same with the matrices not requested


@pytest.mark.parametrize("n", [1025, 8192])
def test_cluster_case_equals_its_closed_form(ctx, n):
    case = cc.cluster_case(n, k=5)
    d = cc.run_device(ctx, case, matrices=False, place="device")
    assert d["rc"] == 0, d["error"]
    for got, want in zip((d["times_checked"], d["cum_inlier"], d["cum_outlier_times"], d["decisions"]), cc.closed_form_clusters(case)):
        assert np.array_equal(got.astype(np.int64), want)


def test_input_forms_places_and_flags(ctx):
    case = cc.realistic_case(129, 0.3, consistent=True, seed=129)
    h = host(case)
    hf = host(cc.with_record_transforms(case))
    for place in ("host", "device", "mixed"):
        assert_equal(cc.run_device(ctx, case, place=place), h, place)
        for rf in (64, 72, 128):      # the records are built in numpy; every word but the twelve upper entries of T is NaN
            assert_equal(cc.run_device(ctx, case, form=rf, place=place), hf, (place, rf))
    base = cc.exact_case(65, seed=4)
    for name, fl in (("null", None), ("all", np.ones(65, np.int32)), ("alternating", (np.arange(65) % 2).astype(np.int32)), ("bit1", np.full(65, 2, np.int32))):
        c = dict(base); c["flags"] = fl; c["name"] = "flags_" + name
        assert_equal(cc.run_device(ctx, c, place="mixed"), host(c), c["name"])
    # only bit 0 counts
    assert np.array_equal(bits(host(dict(base, flags=np.full(65, 2, np.int32), name="flags_bit1"))["te"]), bits(host(dict(base, flags=None, name="flags_null"))["te"]))


def test_seven_calls_accumulate_as_on_the_host(ctx):
    case = cc.cluster_case(65, k=3, counters=[np.zeros(65, np.int32)] * 3)
    dc = hc = case["counters"]
    for call in range(1, 8):
        d = cc.run_device(ctx, case, matrices=False, counters=dc, place="device" if call % 2 else "host")
        h = cc.run_host(case, matrices=False, counters=hc)
        assert_equal(d, h, call, matrices=False)
        dc = [d[k] for k in COUNTERS[:3]]; hc = [h[k] for k in COUNTERS[:3]]
        want = cc.closed_form_clusters(case, calls=call)
        assert np.array_equal(d["decisions"].astype(np.int64), want[3]) and np.array_equal(d["cum_inlier"].astype(np.int64), want[1])
        assert (d["decisions"] == 0).all() == (call < 5)                        # skipped four times, then the vote
    assert set(d["decisions"].tolist()) <= {1, 2}


def test_errors_and_refusals(ctx):
    from g2o_frontend_amd import api
    L = ctx._L
    case = cc.nan_case()
    n = case["n"]
    # the empty column leaves device-resident counters and decisions untouched
    d = cc.run_device(ctx, case, place="device")
    assert d["rc"] == 1 and ("column %d" % case["nan_at"]) in d["error"], d
    for k, a in zip(COUNTERS[:3], case["counters"]):
        assert d[k].tobytes() == np.asarray(a, np.int32).tobytes()
    assert (d["decisions"] == -7).all()
    d = cc.run_device(ctx, case, place="host", matrices=False)
    assert d["rc"] == 1 and (d["decisions"] == -7).all() and all(np.array_equal(d[k], a) for k, a in zip(COUNTERS[:3], case["counters"]))
    h = cc.run_host(case)
    assert h["rc"] == 1 and h["empty_column"] == case["nan_at"]
    # a good call afterwards is not affected by the flag word of the failed one
    good = cc.exact_case(65, seed=2)
    assert_equal(cc.run_device(ctx, good), host(good), "after the error")
    # refusals: nothing written
    ok = cc.cluster_case(5)
    for params, rc in (((0.25, 2.2, 5), 1), ((0.0, 0.26, 5), 1)):
        d = cc.run_device(ctx, ok, params=params)
        assert d["rc"] == rc and (d["decisions"] == -7).all() and (d["te"] == -1).all(), params
    p = cc.params_struct(ok["params"])
    tc = cc.colmajor(ok["tc"]); dec = np.full(5, -7, np.int32); rec = cc.records_of(ok, 64)
    cnt = np.full((3, 5), 3, np.int32)                                         # the three counters: rows of one array
    call = lambda n, tr, records, rf, tcp=tc, c0=cnt[0]: L.pwn_hip_validate_relations(ctx.h, C.byref(p), n, cc.vp(tcp), cc.vp(tc), cc.vp(tr), cc.vp(records), rf, None,
                                                                                       cc.vp(c0), cc.vp(cnt[1]), cc.vp(cnt[2]), cc.vp(dec), None, None)
    assert call(0, tc, None, 0) == 0                                           # n == 0: a no-op
    assert call(8193, tc, None, 0) == 6                                        # beyond PWN_HIP_CONSENSUS_MAX_RELATIONS
    assert call(5, tc, rec, 64) == 1 and call(5, None, None, 0) == 1           # both, neither
    assert call(5, None, rec, 65) == 1 and call(5, None, rec, 0) == 1          # another record size
    assert call(5, tc, None, 0, tcp=None) == 1 and call(5, tc, None, 0, c0=None) == 1
    assert (cnt == 3).all() and (dec == -7).all()
    assert call(5, tc, None, 0) == 0                                           # five identical relations: each gains 1 check and 5 x 5 inlier votes
    assert (cnt[0] == 4).all() and (cnt[1] == 28).all() and (cnt[2] == 3).all() and (dec == 0).all()


def test_stage_names(ctx):
    ctx.check(ctx._L.pwn_hip_set_profiling(ctx.h, 1))
    try:
        assert cc.run_device(ctx, cc.cluster_case(129))["rc"] == 0
        for stage in ("consensus_prepare", "consensus_errors", "consensus_count", "consensus_commit"):
            ms, launches = ctx.stage_ms(stage)
            assert launches == 1 and ms > 0, stage
    finally:
        ctx.check(ctx._L.pwn_hip_set_profiling(ctx.h, 0))


def test_batch_calls_are_unaffected(ctx):
    """one pwn_hip_align_batch_records call before and after a validation returns the same records bit for bit: the validation's scratch does
    not alias the pair arrays"""
    from conftest import case_params, make_depth_pair
    from test_gpu_parity import gpu_objects
    from g2o_frontend_amd import api
    rows, cols, K, conv, _ = case_params("small")
    ref, cur, _, _, _ = make_depth_pair("small", 1)
    _, converter, aligner = gpu_objects(ctx, "small")
    gref, gcur = api.Cloud(ctx, rows * cols), api.Cloud(ctx, rows * cols)
    converter.compute(gref, ref); converter.compute(gcur, cur)
    before = np.zeros((1, 64), np.float32); after = np.zeros((1, 64), np.float32)
    aligner.alignBatchRecords([gref], [gcur], before)
    assert cc.run_device(ctx, cc.cluster_case(513), place="mixed")["rc"] == 0
    aligner.alignBatchRecords([gref], [gcur], after)
    assert before[0, 18] > 0 and np.array_equal(before.view(np.uint32), after.view(np.uint32))


@pytest.mark.parametrize("consistent", [False, True])
def test_python_mirror(ctx, consistent):
    """api.MapCloser.validatePartitions on relations made from a case, half of them stored the other way round (nodes[1] in current, the
    transform inverted): committed, removed and the write-back equal the host function's on the oriented triples, three validations in a row"""
    from g2o_frontend_amd import api
    case = cc.realistic_case(65, 0.3, consistent=False, seed=11)
    n = case["n"]
    cur_nodes, oth_nodes, rels = {}, {}, []
    node = lambda pool, T: pool.setdefault(T.tobytes(), api.MapNode(len(pool), T))
    swapped = (np.arange(n) % 2).astype(np.int32)
    for k in range(n):
        a, b = node(cur_nodes, case["tc"][k]), node(oth_nodes, case["to"][k])
        T = case["tr"][k]
        rels.append(dict(nodes=(b, a), transform=api._iso_inverse_d(T)) if swapped[k] else dict(nodes=(a, b), transform=T))
    closers = [api.MapCloser(ctx, consistent=consistent), api.MapCloser(None, consistent=consistent)]
    for mc in closers:
        mc.setConsensusMinTimesCheckedThreshold(2)
        for r in rels:
            mc.addRelation(dict(r))
    oriented = dict(case, tr=np.stack([r["transform"] for r in rels]), flags=swapped ^ (1 if consistent else 0), params=(cc.THR_T, cc.THR_R, 2),
                    name="mirror_%d" % consistent)
    cnt = oriented["counters"]
    for call in range(3):
        h = cc.run_host(oriented, matrices=False, counters=cnt)
        assert h["rc"] == 0
        for mc in closers:
            live = mc.relations()
            committed, removed = mc.validatePartitions(list(oth_nodes.values()), list(cur_nodes.values()))
            assert [any(r is q for q in committed) for r in live] == (h["decisions"] == 1).tolist()
            assert [any(r is q for q in removed) for r in live] == (h["decisions"] == 2).tolist()
            assert [r["consensusCumInlier"] for r in live] == h["cum_inlier"].tolist()
            assert [r["consensusCumOutlierTimes"] for r in live] == h["cum_outlier_times"].tolist()
            assert [r["consensusTimeChecked"] for r in live] == h["times_checked"].tolist()
            assert len(mc.relations()) == len(live) - len(removed)
        keep = h["decisions"] != 2
        if call == 1:
            assert (h["decisions"] != 0).all()                                  # times_checked has reached the minimum of 2
        oriented = dict(oriented, **{k: oriented[k][keep] for k in ("tc", "to", "tr", "flags")}, n=int(keep.sum()), name="mirror_%d_%d" % (consistent, call))
        cnt = [h[k][keep] for k in COUNTERS[:3]]
        if oriented["n"] == 0:
            break
    # the records form through the mirror: the transforms of the surviving relations as a closer call's records, on the device
    mc = closers[0]
    live = mc.relations()
    if live:
        rec = np.full((len(live), 72), np.nan, np.float32)
        rec[:, :16] = np.stack([np.asarray(r["transform"]).T.reshape(16) for r in live]).astype(np.float32)
        h = cc.run_host(cc.with_record_transforms(oriented), matrices=False, counters=cnt)
        mc.validatePartitions(list(oth_nodes.values()), list(cur_nodes.values()), records=api.DeviceBuffer(ctx, rec))
        assert h["rc"] == 0 and [r["consensusCumInlier"] for r in live] == h["cum_inlier"].tolist()
        assert [r["consensusCumOutlierTimes"] for r in live] == h["cum_outlier_times"].tolist()
