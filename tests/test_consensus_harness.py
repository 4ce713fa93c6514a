"""The two mirrors of MapCloser::validatePartitions held together: api.MapCloser runs three consecutive validations of a partition pair on the
device and writes poses, relations, counters and its results to a file; tools/pwn_hip_consensus_check runs the C++ mirror
(host/pwn_hip.hpp) on the same input and must print " 0 differences"."""
import os
import struct
import subprocess

import numpy as np
import pytest

import consensus_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("consistent", [False, True])
def test_cpp_mirror_equals_python_mirror(tmp_path, consistent):
    from g2o_frontend_amd import api
    case = cc.realistic_case(65, 0.3, consistent=False, seed=11)
    n, min_times, validations = case["n"], 2, 3
    rng = np.random.default_rng(5)
    cur, oth = {}, {}
    index = lambda pool, T: pool.setdefault(T.tobytes(), (len(pool), T))[0]
    rel_nodes = [(index(cur, case["tc"][k]), index(oth, case["to"][k])) for k in range(n)]
    swapped = (np.arange(n) % 3 == 1)                                        # stored the other way round: nodes[0] in the other partition
    counters = rng.integers(0, 3, (n, 3)).astype(np.int32); counters[:, 0] = 0
    cur_nodes = [api.MapNode(i, T) for i, T in sorted(cur.values(), key=lambda v: v[0])]
    oth_nodes = [api.MapNode(len(cur) + i, T) for i, T in sorted(oth.values(), key=lambda v: v[0])]
    ctx = api.Context(device=0, max_rows=120, max_cols=160, max_batch=1)
    closer = api.MapCloser(ctx, consistent=consistent)
    closer.setConsensusMinTimesCheckedThreshold(min_times)
    blob = struct.pack("<6i2f", len(cur_nodes), len(oth_nodes), n, int(consistent), min_times, validations, closer.consensusInlierTranslationalThreshold(),
                       closer.consensusInlierRotationalThreshold())
    for node in cur_nodes + oth_nodes:
        blob += np.ascontiguousarray(node.transform(), np.float64).tobytes()
    rels = []
    for k, (a, b) in enumerate(rel_nodes):
        T = api._iso_inverse_d(case["tr"][k]) if swapped[k] else case["tr"][k]
        nodes = (oth_nodes[b], cur_nodes[a]) if swapped[k] else (cur_nodes[a], oth_nodes[b])
        r = dict(nodes=nodes, transform=np.ascontiguousarray(T, np.float64), consensusTimeChecked=int(counters[k, 0]), consensusCumInlier=int(counters[k, 1]),
                 consensusCumOutlierTimes=int(counters[k, 2]), index=k)
        closer.addRelation(r); rels.append(r)
        blob += struct.pack("<3i", 0 if swapped[k] else 1, b if swapped[k] else a, a if swapped[k] else b) + r["transform"].tobytes() + counters[k].tobytes()
    decided = set()
    for v in range(validations):
        live = closer.relations()
        committed, removed = closer.validatePartitions(oth_nodes, cur_nodes)
        blob += struct.pack("<i", len(live))
        for r in live:
            d = 2 if any(r is q for q in removed) else 1 if any(r is q for q in committed) else 0
            decided.add(d)
            blob += struct.pack("<5i", r["index"], d, r["consensusTimeChecked"], r["consensusCumInlier"], r["consensusCumOutlierTimes"])
    ctx.close()
    assert decided == ({0, 1, 2} if consistent else {0, 2})                   # the file exercises every decision the orientation can produce
    path = str(tmp_path / "consensus.bin")
    with open(path, "wb") as fh:
        fh.write(blob)
    r = subprocess.run([os.path.join(ROOT, "tools", "pwn_hip_consensus_check"), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 differences" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
