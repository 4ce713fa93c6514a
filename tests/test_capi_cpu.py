"""No-GPU checks of the product: the C-ABI library loads and exports every symbol include/pwn_hip.h declares,
fails loudly without a device, the host-side parameter plumbing mirrors the reference defaults, and the product
package never touches the oracle."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = ""
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):      # pwn_hip.h (the boundary) and pwn_hip_testing.h (test hooks)
        if h.endswith(".h"):
            src += open(os.path.join(ROOT, "include", h)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pwn_hip_[a-z0-9_]+)\s*\(", src)))


def test_test_hooks_are_not_in_the_boundary_header():
    src = open(os.path.join(ROOT, "include", "pwn_hip.h")).read()
    assert "debug_" not in src and "pwn_hip_debug_withhold_carry" in open(os.path.join(ROOT, "include", "pwn_hip_testing.h")).read()


def test_boundary_headers_are_plain_c():
    """The boundary is a C ABI (cgo / JNI / ctypes bind it): a C99 compiler takes both headers as they are, warnings on."""
    import subprocess
    for h in ("pwn_hip.h", "pwn_hip_testing.h"):
        r = subprocess.run(["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", os.path.join(ROOT, "include", h)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]


def test_library_exports_every_declared_symbol():
    from g2o_frontend_amd import _lib
    names = declared_symbols()
    assert len(names) >= 30
    L = C.CDLL(_lib.LIB_PATH)
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    # and the Python prototypes cover the header exactly
    assert sorted(_lib.PROTOTYPES) == names
    _lib.lib()


def test_struct_layouts_match_header_sizes():
    """ctypes mirrors of the parameter / result structs have the sizes the C compiler gives the header's structs."""
    import subprocess, tempfile
    from g2o_frontend_amd import _lib
    prog = r'''
#include <stdio.h>
#include "pwn_hip.h"
int main(void) { printf("%zu %zu %zu\n", sizeof(pwn_hip_converter_params), sizeof(pwn_hip_aligner_params), sizeof(pwn_hip_align_result)); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    assert [int(x) for x in out] == [C.sizeof(_lib.ConverterParams), C.sizeof(_lib.AlignerParams), C.sizeof(_lib.AlignResult)]


def test_defaults_are_the_reference_class_defaults():
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    cp = _lib.ConverterParams(); L.pwn_hip_default_converter_params(C.byref(cp))
    ap = _lib.AlignerParams(); L.pwn_hip_default_aligner_params(C.byref(ap))
    assert list(cp.K) == [1, 0, 0, 0, 1, 0, 0.5, 0.5, 1]                              # pinholepointprojector.cpp:6-9
    assert (round(cp.min_distance, 6), cp.max_distance) == (0.01, 6.0)                 # pointprojector.cpp:9-10
    assert (round(cp.world_radius, 6), cp.min_image_radius, cp.max_image_radius, cp.min_points) == (0.1, 10, 30, 50)
    assert round(cp.stats_curvature_threshold, 6) == 0.02 and list(cp.point_flat_diag) == [1000, 1, 1] and list(cp.normal_flat_diag) == [100, 100, 100]
    assert list(cp.sensor_offset) == list(np.eye(4).ravel())
    assert (ap.inlier_distance_threshold, ap.inlier_curvature_ratio_threshold, ap.inlier_max_chi2) == (0.5, np.float32(1.3), 9000.0)
    assert abs(ap.inlier_normal_angular_threshold - np.cos(np.pi / 6)) < 1e-7
    assert (ap.robust_kernel, ap.outer_iterations, ap.inner_iterations) == (1, 10, 1)  # linearizer.cpp:14, aligner.cpp:19-20


def test_helpers_run_on_the_host_and_match_the_oracle(oracle):
    """The SE(3) / projector-matrix helpers are host code of the product; same bits as the oracle."""
    from g2o_frontend_amd import api
    rng = np.random.default_rng(0)
    for _ in range(50):
        v = np.concatenate([rng.normal(size=3), rng.uniform(-0.3, 0.3, size=3)]).astype(np.float32)
        T = api.v2t(v)
        assert np.array_equal(T, oracle.v2t(v)) and np.array_equal(api.t2v(T), oracle.t2v(T))
        p = api.PinholePointProjector(); p.setCameraMatrix([[525, 0, 319.5], [0, 525, 239.5], [0, 0, 1]]); p.setTransform(T)
        for a, b in zip(p.matrices(), oracle.projector_matrices((525, 525, 319.5, 239.5), T)):
            assert np.array_equal(a, b)
    for n in range(300):                                                    # rotations beyond 120 degrees: the trace <= 0 branches of t2v
        q = rng.normal(size=3); q *= rng.uniform(0.87, 0.9999) / np.linalg.norm(q)
        if n % 3 == 0: q[n // 3 % 3] *= 8; q *= rng.uniform(0.87, 0.9999) / np.linalg.norm(q)     # one dominant axis each
        T = api.v2t(np.concatenate([rng.normal(size=3), q]).astype(np.float32))
        assert np.array_equal(T, oracle.v2t(api.t2v(T) * 0 + np.concatenate([T[:3, 3], q]).astype(np.float32)))
        assert np.array_equal(api.t2v(T).view(np.uint32), oracle.t2v(T).view(np.uint32))


def test_ldlt_host_compilation_matches_the_oracle(oracle):
    """The 6x6 pivoted LDLT the device runs in registers (every index a compile-time constant, pivot swaps dispatched on the pivot
    row): its host compilation against the oracle's loop form, bit for bit -- well conditioned systems, the aligner's
    H + 1001 I shape, every pivot order, rank-deficient and all-zero matrices."""
    from g2o_frontend_amd import api
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(300):
        J = rng.normal(size=(12, 6)); H = (J.T @ J) * 10.0 ** rng.uniform(-3, 6)
        cases.append((H, rng.normal(size=6)))
    for _ in range(100):                                                    # the Gauss-Newton shape: large, badly scaled blocks + damping
        J = rng.normal(size=(40, 6)) * np.array([30, 30, 30, 900, 900, 900]); H = J.T @ J + 1001.0 * np.eye(6)
        cases.append((H, rng.normal(size=6) * 1e4))
    import itertools
    for perm in itertools.permutations(range(6)):                           # every order of the diagonal: every pivot sequence
        d = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0])[list(perm)]
        L = np.tril(rng.normal(size=(6, 6)) * 0.1, -1) + np.eye(6)
        cases.append((L @ np.diag(d) @ L.T, rng.normal(size=6)))
    for r in range(6):                                                      # rank r: the factorisation stops early
        J = rng.normal(size=(r, 6)); cases.append((J.T @ J, rng.normal(size=6)))
    cases.append((np.zeros((6, 6)), np.ones(6)))
    cases.append((np.diag([0, 0, 5.0, 0, 0, 0]), np.arange(6.0)))
    cases.append((-np.eye(6) * 3 + 0.1, np.arange(6.0)))                    # negative definite: LDLT still factors it
    for H, b in cases:
        H = H.astype(np.float32); b = b.astype(np.float32)
        x, xo = api.ldlt_solve6(H, b), oracle.ldlt_solve6(H, b)
        assert np.array_equal(x.view(np.uint32), xo.view(np.uint32)), (H, b, x, xo)


def test_host_mirror_parameter_plumbing():
    from g2o_frontend_amd import api
    p = api.PinholePointProjector(); p.setCameraMatrix([[525, 0, 319.5], [0, 525, 239.5], [0, 0, 1]]); p.setImageSize(480, 640)
    p.scale(0.5)                                                                       # pinholepointprojector.cpp:149-154
    assert p.imageRows() == 240 and p.imageCols() == 320 and p.cameraMatrix()[0, 0] == 262.5 and p.cameraMatrix()[2, 2] == 1
    st = api.StatsCalculatorIntegralImage(); st.setMinImageRadius(3); st.setCurvatureThreshold(0.2)
    conv = api.DepthImageConverterIntegralImage(p, st, api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator())
    cp = conv.params(np.eye(4))
    assert cp.min_image_radius == 3 and abs(cp.stats_curvature_threshold - 0.2) < 1e-7 and cp.K[0] == 262.5 and cp.K[6] == 159.75
    al = api.Aligner.__new__(api.Aligner)
    al.__dict__.update(ctx=None, _projector=None, _linearizer=None, _correspondenceFinder=None)
    with pytest.raises(AssertionError):
        al.params()                                                                    # aligner.cpp:50-52 asserts


def test_no_device_fails_loudly():
    from g2o_frontend_amd import _lib, api
    if _lib.lib().pwn_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.PwnHipError) as e:
        api.Context()
    assert e.value.code == 2 and "no CPU fallback" in str(e.value)


def test_null_arguments_are_status_codes_not_crashes():
    """every entry point that takes a context rejects a null one (and null handles) with PWN_HIP_ERR_INVALID_ARGUMENT -- no device needed"""
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel()); K = (C.c_float * 9)(525, 0, 0, 0, 525, 0, 319.5, 239.5, 1)
    n = C.c_int(0); out = (C.c_float * 16)()
    cases = {
        "pwn_hip_cloud_add": (None, None, None, T),
        "pwn_hip_merge": (None, None, K, T, 0.5, 4.5, 120, 160, 0.1, 0.98, 10.0, C.byref(n), None),
        "pwn_hip_voxelize": (None, None, 0.01, C.byref(n), None),
        "pwn_hip_cloud_save": (None, None, b"/tmp/x.pwn", T, 1, 0),
        "pwn_hip_cloud_load": (None, None, b"/tmp/x.pwn", out),
        "pwn_hip_cloud_gaussians": (None, None, None, 120, 160, None, 0.075, 0.1),
        "pwn_hip_cloud_download_gaussians": (None, None, None, None, None, None, None),
        "pwn_hip_cloud_num_gaussians": (None, None, C.byref(n)),
        "pwn_hip_cloud_transform_in_place": (None, None, T),
        "pwn_hip_ctx_set_concurrency": (None, 2),
        "pwn_hip_ctx_set_omega_storage": (None, 1),
        "pwn_hip_cloud_omega_storage": (None, None, C.byref(n)),
        "pwn_hip_ctx_set_subbatch": (None, 64, 64),
        "pwn_hip_align": (None, None, None, None, None),
        "pwn_hip_align_batch_records": (None, None, 1, None, None, None, None, 0, None, None),
        "pwn_hip_convert_align_batch_u16": (None, None, None, 1, None, None, 0.001, 120, 160, None, None, None, None, 0, None, None),
        "pwn_hip_convert": (None, None, None, 120, 160, None, None, None, 0),
    }
    for name, args in cases.items():
        rc = getattr(L, name)(*args)
        assert rc == 1, (name, rc)
        assert L.pwn_hip_last_error_string(None)


def test_product_does_not_import_the_oracle():
    """The oracle is test infrastructure: nothing under g2o_frontend_amd/ or include/ may reference it."""
    pat = re.compile(r"(from\s+oracle|import\s+oracle|oracle\.|pwn_oracle|libpwn_oracle|orc_[a-z_]+\()")
    for base in ("g2o_frontend_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".h", ".hip", ".cpp", ".hpp")):
                    txt = open(os.path.join(dirpath, f)).read()
                    assert not pat.search(txt), os.path.join(dirpath, f)


def test_bench_imports_the_oracle_only_in_the_cpu_baseline_leg():
    """bench.py's GPU-driving process never imports the checker: `from oracle import ...` may appear only inside the two functions of the
    cpu_baseline child process (round-2 review: the parameter tables now live in g2o_frontend_amd/conf.py)."""
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    allowed = {"_cpu_worker", "cpu_baseline_child"}

    def visit(node, fn):
        for ch in ast.iter_child_nodes(node):
            name = ch.name if isinstance(ch, (ast.FunctionDef, ast.AsyncFunctionDef)) else fn
            if isinstance(ch, ast.ImportFrom) and (ch.module or "").split(".")[0] == "oracle":
                assert fn in allowed, (fn, ch.lineno)
            if isinstance(ch, ast.Import):
                assert not any(a.name.split(".")[0] == "oracle" for a in ch.names) or fn in allowed, (fn, ch.lineno)
            visit(ch, name)
    visit(tree, None)


def test_binding_sources_use_names_the_reference_headers_declare():
    """bindings/pwn_hip/ cannot be compiled here (Eigen3 + OpenCV missing): at least every member and accessor it uses must exist in the
    reference headers it is written against (tools/check_binding_names.py; a syntax check, not parity evidence).  The headers' names are read
    from tests/golden/reference_names.json (tests/golden/make_reference_names.py)."""
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_binding_names.py"), os.path.join(ROOT, "tests", "golden", "reference_names.json")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "MISSING" not in out.stdout and " 0 members" not in out.stdout and " 0 methods" not in out.stdout, out.stdout


def test_packed_xyz_records_are_accessed_as_12_byte_words():
    """The 12-byte point records and information-matrix rows are accessed through a 4-byte-aligned vector type (pwn_kernels.h: v3f): the
    gfx950 code must contain dwordx3 accesses for them and no 16-byte store other than the one of the 16-byte (normal, curvature) record --
    a store widened to dwordx4 would overwrite the next point's x / the next matrix row (round-2 advisor finding)."""
    import struct
    import subprocess
    import tempfile
    from g2o_frontend_amd import _lib
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not installed")
    blob = open(_lib.LIB_PATH, "rb").read()
    i = blob.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert i >= 0
    n = struct.unpack_from("<Q", blob, i + 24)[0]; off = i + 32
    code = None
    for _ in range(n):
        o, sz, tl = struct.unpack_from("<QQQ", blob, off); name = blob[off + 24: off + 24 + tl].decode(); off += 24 + tl
        if "gfx950" in name:
            code = blob[i + o: i + o + sz]
    assert code, "no gfx950 code object in the library"
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code); f.flush()
        asm = subprocess.run([objdump, "-d", f.name], capture_output=True, text=True).stdout
    counts, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1); continue
        for ins in ("global_store_dwordx4", "global_store_dwordx3", "global_load_dwordx3"):
            if cur and ins in line:
                counts[(cur, ins)] = counts.get((cur, ins), 0) + 1
    def get(sub, ins): return sum(v for (k, i2), v in counts.items() if i2 == ins and re.search(sub, k))
    assert get(r"7k_statsE", "global_store_dwordx3") >= 4 and get(r"7k_statsE", "global_store_dwordx4") <= 1      # P3 + 3 rows; Nc is the one float4
    assert get(r"20k_unproject_integralE", "global_store_dwordx4") == 0 and get(r"25k_unproject_integral_rowsE", "global_store_dwordx4") == 0
    assert get(r"16k_corr_linearizeI", "global_load_dwordx3") >= 10


def _gfx950_code_object():
    import struct
    from g2o_frontend_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    i = blob.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert i >= 0
    n = struct.unpack_from("<Q", blob, i + 24)[0]; off = i + 32
    for _ in range(n):
        o, sz, tl = struct.unpack_from("<QQQ", blob, off); name = blob[off + 24: off + 24 + tl].decode(); off += 24 + tl
        if "gfx950" in name:
            return blob[i + o: i + o + sz]
    raise AssertionError("no gfx950 code object in the library")


def test_kernel_resources_of_the_hot_and_the_serial_kernels():
    """Register / scratch / LDS budget of the kernels whose speed depends on it, read from the code object's metadata.  Round 3 lost 8 us per
    64-pair launch of k_solve_update (10.5 -> 18 us) to a refactoring that made the compiler spill 68 bytes and promote an array to 16 KB of LDS;
    nothing but a kernel trace showed it.  Bars: no scratch anywhere on the path's kernels; k_solve_update's LDS is its reduction buffers only;
    the fused pass keeps its 5 waves per SIMD (<= 96 VGPRs... 102 is the allocation granule's limit for 5), k_stats its 8 (<= 64)."""
    import subprocess
    import tempfile
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
        elif cur is not None and key in ("private_segment_fixed_size", "vgpr_count", "sgpr_count"):
            cur[{"private_segment_fixed_size": "scratch", "vgpr_count": "vgpr", "sgpr_count": "sgpr"}[key]] = int(val)
    def one(sub):
        hits = [(k, v) for k, v in kernels.items() if re.search(sub, k)]
        assert hits, (sub, sorted(kernels)[:5])
        return hits
    for sub in (r"14k_solve_updateE", r"7k_statsE", r"16k_corr_linearizeI", r"20k_corr_linearize_latI", r"9k_projectI", r"20k_unproject_integralE",
                r"25k_unproject_integral_rowsE", r"15k_integral_colsE", r"13k_strip_countI"):
        for name, r in one(sub):
            assert r["scratch"] == 0, (name, r)
    (name, r), = one(r"14k_solve_updateE")
    assert r["lds"] <= 4096 and r["vgpr"] <= 96, (name, r)
    for name, r in one(r"7k_statsE"):
        assert r["vgpr"] <= 64, (name, r)
    for name, r in one(r"16k_corr_linearizeILb1ELb0E"):
        assert r["vgpr"] <= 102, (name, r)


def test_product_sources_carry_no_compile_time_or_environment_switches():
    """The kernels' bit-exactness is the product: the sources under g2o_frontend_amd/csrc hold no `#if` / `#ifdef` / `#ifndef` block (round 4's
    header had 38, several of them timing experiments that produce wrong results when defined) and read no environment variable; the build
    passes no -D flag.  Experiments live in history and in docs/experiments.md."""
    from g2o_frontend_amd import build
    d = os.path.join(ROOT, "g2o_frontend_amd", "csrc")
    for f in sorted(os.listdir(d)):
        text = open(os.path.join(d, f)).read()
        for n, line in enumerate(text.splitlines(), 1):
            assert not re.match(r"\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", line), (f, n, line)
        assert "getenv" not in text, f
    assert not [x for x in build.FLAGS if x.startswith("-D")]


def test_runtime_allocation_calls_live_in_the_buffer_type_and_the_caller_facing_entry_points_only():
    """The library's own device and page-locked memory -- a cloud's arrays included -- is owned by pwn_buffers.h's buffer type (a member that
    frees itself: no list in pwn_hip_ctx_destroy or in a cloud's destruction to forget it in).  The runtime's four allocation / free calls may
    appear only there and in the four entry points that hand memory to the caller; a raw call anywhere else fails here."""
    allowed = {"pwn_hip_device_alloc", "pwn_hip_device_free", "pwn_hip_host_alloc", "pwn_hip_host_free"}
    call = re.compile(r"\bhip(Malloc|Free|HostMalloc|HostFree)\s*\(")
    d = os.path.join(ROOT, "g2o_frontend_amd", "csrc")
    seen = set()
    for f in sorted(os.listdir(d)):
        text = re.sub(r"//[^\n]*", "", open(os.path.join(d, f)).read())
        if f == "pwn_buffers.h":
            assert len(call.findall(text)) == 4, "the buffer type calls each of the four once"
            continue
        fn = None
        for n, line in enumerate(text.splitlines(), 1):
            m = re.match(r"(?![#}])\S.*?(\w+)\s*\(", line)                    # a definition starts in column 0 and does not end in ';'
            if m and not line.rstrip().endswith(";"):
                fn = m.group(1)
            if call.search(line):
                assert fn in allowed, (f, n, fn, line.strip())
                seen.add(fn)
    assert seen == allowed, sorted(allowed - seen)


def test_a_clouds_content_record_is_written_by_its_own_functions_only():
    """What a cloud's arrays mean -- size, Stats, Gaussians, index image and its key -- is the CloudContent member of pwn_hip_cloud.  Its fields are
    assigned inside that struct and nowhere else in csrc/: the transitions (replace, commit, edit) and the named setters call its functions, nothing
    takes a writable reference to it, and the loose fields it replaced are gone."""
    d = os.path.join(ROOT, "g2o_frontend_amd", "csrc")
    text = {f: re.sub(r"//[^\n]*", "", open(os.path.join(d, f)).read()) for f in sorted(os.listdir(d))}
    capi = text["pwn_hip_capi.hip"]
    m = re.search(r"\nstruct CloudContent \{\n.*?\n\};\n", capi, flags=re.S)
    assert m and capi.count("struct CloudContent") == 1
    names = ["n", "stats", "n_gauss", "idx_valid", "idx_key"]
    decls = re.findall(r"^  (?:int|bool) (\w+) = \w+;| IndexKey (\w+);", m.group(0), flags=re.M)
    assert sorted(a or b for a, b in decls) == sorted(names), decls
    text["pwn_hip_capi.hip"] = capi.replace(m.group(0), "\n")
    write = re.compile(r"\bcontent\s*(?:\.\s*(?:%s)\s*)?(?:=(?!=)|[-+*/|&^]=|\+\+|--)|(?:\+\+|--)\s*[\w>.-]*\bcontent\b" % "|".join(names))
    for f, t in text.items():
        for n, line in enumerate(t.splitlines(), 1):
            assert not write.search(line), (f, n, line.strip())
            assert not re.search(r"(?<!const )CloudContent\s*[&*]", line), (f, n, line.strip())
            assert not re.search(r"\b(n_host|has_stats)\b|->\s*(n_gauss|idx_valid|idx_key)\b", line), (f, n, line.strip())
    assert len(re.findall(r"\bCloudContent\b", text["pwn_hip_capi.hip"])) == 1, "one member of that type, in pwn_hip_cloud"


def test_single_point_projector_forms_against_the_numpy_model():
    """PinholePointProjector::project(x, y, f, p) / unProject(p, x, y, d) / projectInterval (pinholepointprojector.h:174,187,200) are host code of the
    library (no GPU): against the numpy statement of the reference's lines (tests/numpy_reference_model.py), point by point, bit for bit."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy_reference_model as M
    from g2o_frontend_amd import api, synth
    K = synth.K_VGA
    rng = np.random.default_rng(5)
    T = synth.v2t(np.array([0.04, -0.03, 0.05, 0.01, -0.015, 0.02])).astype(np.float32)
    proj = api.PinholePointProjector()
    proj.setCameraMatrix([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]); proj.setTransform(T); proj.setMinDistance(0.5); proj.setMaxDistance(4.5)
    KRt, iKRt, _ = M.projector_matrices(K, T)
    # unProject: pixels of a synthetic depth image (out-of-range depths included)
    depth = rng.uniform(0.2, 5.0, (12, 16)).astype(np.float32)
    valid, x, y, z = M.unproject(depth, iKRt, 0.5, 4.5)
    P = []
    for r in range(12):
        for c in range(16):
            ok, p = proj.unProjectPixel(c, r, depth[r, c])
            assert ok == bool(valid[r, c])
            if ok:
                assert np.array_equal(p.view(np.uint32), np.array([x[r, c], y[r, c], z[r, c]], np.float32).view(np.uint32)), (r, c)
                P.append(p)
    # project: those points back through the same projector; the model's image is what the single-point results scatter to
    P = np.array(P, np.float32)
    x_, y_, z_ = P[:, 0], P[:, 1], P[:, 2]
    row = lambda k: ((KRt[k, 0] * x_ + KRt[k, 1] * y_) + KRt[k, 2] * z_) + KRt[k, 3] * np.float32(1.0)      # noqa: E731
    ix, iy, d = row(0), row(1), row(2)
    for i in range(len(P)):
        ok, px, py, pd = proj.projectPoint(P[i])
        assert np.float32(pd).view(np.uint32) == d[i].view(np.uint32)
        assert ok == (not (d[i] < np.float32(0.5) or d[i] > np.float32(4.5)))
        if ok:
            inv = np.float32(1.0) / d[i]
            assert (px, py) == (int(M.roundf(ix[i] * inv)), int(M.roundf(iy[i] * inv))), i
    # projectInterval
    itv = M.intervals(depth, valid, K, 0.1)
    for r in range(12):
        for c in range(16):
            assert proj.projectInterval(c, r, depth[r, c], 0.1) == int(itv[r, c]), (r, c)


def test_flat_cloud_buffers_are_checked_before_they_reach_the_library():
    """Cloud.exportFlat / importFlat hand raw pointers to kernels on the context's device (advisor finding, round 5): a strided view, another
    element type or a read-only destination is refused in Python, like the records buffers are."""
    from types import SimpleNamespace
    from g2o_frontend_amd import api
    ctx = SimpleNamespace(device=0)
    ok = np.zeros(1024, np.uint8)
    api._check_flat(ok, ctx, writable=True)
    ro = np.zeros(1024, np.uint8); ro.setflags(write=False)
    api._check_flat(ro, ctx, writable=False)                       # a read-only source is fine
    for bad in (ro, np.zeros(1024, np.float32), np.zeros((64, 64), np.uint8)[:, ::2]):
        with pytest.raises(ValueError):
            api._check_flat(bad, ctx, writable=True)
    with pytest.raises(TypeError):
        api._check_flat([0] * 16, ctx, writable=False)
    import torch
    t = torch.zeros(1024, dtype=torch.uint8)
    api._check_flat(t, ctx, writable=True)                         # a host tensor
    with pytest.raises(ValueError):
        api._check_flat(torch.zeros(1024, dtype=torch.float32), ctx, writable=True)
    with pytest.raises(ValueError):
        api._check_flat(torch.zeros(64, 64, dtype=torch.uint8)[:, ::2], ctx, writable=True)


def test_library_default_storage_is_documented_consistently():
    """the header, the Python mirror and the bench agree on the default storage of the point information matrices (sym6 since round 6)"""
    from g2o_frontend_amd import api
    import bench
    h = open(os.path.join(ROOT, "include", "pwn_hip.h")).read()
    assert "PWN_HIP_OMEGA_SYM6 (the default since round 6)" in h
    assert api.Context.DEFAULT_OMEGA_STORAGE == "sym6"
    assert bench.parse([]).omega_storage == "sym6"
    src = open(os.path.join(ROOT, "g2o_frontend_amd", "csrc", "pwn_hip_capi.hip")).read()
    assert "int omega_sym = 1;" in src
