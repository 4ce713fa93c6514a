"""k_pair_statistics (Aligner::_computeStatistics' 6x6 math on the device) keeps its matrices in LDS: no scratch, at most 4 KB of LDS -- read from
the gfx950 code object's metadata as tests/test_capi_cpu.py::test_kernel_resources_of_the_hot_and_the_serial_kernels does for the other kernels."""
import os
import re
import subprocess
import tempfile

import pytest

from test_capi_cpu import _gfx950_code_object


def test_pair_statistics_kernel_has_no_scratch_and_little_lds():
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not installed")
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(_gfx950_code_object()); f.flush()
        notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2)
        if key == "group_segment_fixed_size":
            cur = {"lds": int(val)}
        elif cur is not None and key == "name":
            kernels[val] = cur
        elif cur is not None and key == "private_segment_fixed_size":
            cur["scratch"] = int(val)
    hits = [(k, v) for k, v in kernels.items() if re.search(r"17k_pair_statisticsE", k)]
    assert len(hits) == 1, sorted(kernels)[:5]
    name, r = hits[0]
    assert r["scratch"] == 0 and 0 < r["lds"] <= 4096, (name, r)
    for sub in (r"14k_pack_recordsE", r"22k_pack_closure_recordsE"):
        (name, r), = [(k, v) for k, v in kernels.items() if re.search(sub, k)]
        assert r["scratch"] == 0 and r["lds"] == 0, (name, r)
