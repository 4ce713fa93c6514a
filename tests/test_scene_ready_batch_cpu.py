"""No-GPU checks of the scene-ready batch conversion (pwn_hip_convert_batch_ex): the library exports the new symbols, the boundary header declares
them as plain C, a null context is a status code with an error string, the extras' defaults are the projector's (pinholepointprojector.cpp:10-11),
the ctypes mirror of the struct has the header's size, and the mirrors offer the option where the issue puts it."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pwn_hip_convert_batch_ex", "pwn_hip_default_convert_extras")


def test_library_exports_the_new_symbols_and_the_header_declares_them_as_plain_c():
    from g2o_frontend_amd import _lib
    header = open(os.path.join(ROOT, "include", "pwn_hip.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
    assert "typedef struct pwn_hip_convert_extras" in header
    # the store-form hook is a test hook: in the testing header, not in the boundary
    assert "pwn_hip_debug_set_gaussian_stores" in open(os.path.join(ROOT, "include", "pwn_hip_testing.h")).read()
    assert hasattr(L, "pwn_hip_debug_set_gaussian_stores")
    prog = '#include "pwn_hip.h"\nint main(void) { pwn_hip_convert_extras e; pwn_hip_default_convert_extras(&e); return e.keep_stats + e.gaussians; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"),
                            os.path.join(d, "t.c"), "-L", os.path.dirname(_lib.LIB_PATH), "-lpwn_hip", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-800:]
        assert subprocess.run([os.path.join(d, "t")]).returncode == 0


def test_null_context_is_a_status_code_with_an_error_string():
    from g2o_frontend_amd import _lib
    L = _lib.lib()
    ex = _lib.ConvertExtras(1, 1, 0.075, 0.1)
    for extras in (None, C.byref(ex)):
        for step in (0, 2):
            for raw in (0, 1):
                rc = L.pwn_hip_convert_batch_ex(None, None, None, raw, 0.001, 1, 120, 160, step, 0.01, extras, None)
                assert rc == 1, (step, raw, rc)
                assert L.pwn_hip_last_error_string(None)
    assert L.pwn_hip_debug_set_gaussian_stores(None, 1) == 1 and L.pwn_hip_last_error_string(None)
    L.pwn_hip_default_convert_extras(None)      # a null struct is ignored, not dereferenced


def test_default_extras_are_off_with_the_projectors_noise_model():
    import numpy as np
    from g2o_frontend_amd import _lib, api
    L = _lib.lib()
    e = _lib.ConvertExtras(7, 7, -1.0, -1.0)
    L.pwn_hip_default_convert_extras(C.byref(e))
    assert (e.keep_stats, e.gaussians) == (0, 0)
    assert (np.float32(e.baseline), np.float32(e.alpha)) == (np.float32(0.075), np.float32(0.1))      # pinholepointprojector.cpp:10-11
    p = api.PinholePointProjector()
    assert (np.float32(p.baseline()), np.float32(p.alpha())) == (np.float32(e.baseline), np.float32(e.alpha))


def test_struct_size_matches_the_header():
    from g2o_frontend_amd import _lib
    prog = '#include <stdio.h>\n#include "pwn_hip.h"\nint main(void) { printf("%zu\\n", sizeof(pwn_hip_convert_extras)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        assert int(subprocess.check_output([os.path.join(d, "t")]).decode()) == C.sizeof(_lib.ConvertExtras) == 16
    assert [f[0] for f in _lib.ConvertExtras._fields_] == ["keep_stats", "gaussians", "baseline", "alpha"]


def test_mirrors_offer_the_option_and_default_to_lean():
    from g2o_frontend_amd import api
    for fn in (api.DepthImageConverterIntegralImage.computeBatch, api.PwnMatcherBase.makeCloudBatch, api.PwnMatcherBase.makeCloud):
        sig = inspect.signature(fn)
        assert sig.parameters["keep_stats"].default is False and sig.parameters["gaussians"].default is False, fn
    assert inspect.signature(api.CloudCache.__init__).parameters["sceneReady"].default is False
    assert "sceneReady" in api.PwnMerger.__doc__
    conv = api.DepthImageConverterIntegralImage(api.PinholePointProjector(), api.StatsCalculatorIntegralImage(), api.PointInformationMatrixCalculator(),
                                                api.NormalInformationMatrixCalculator())
    assert conv.extras(False, False) is None
    e = conv.extras(True, False)
    assert (e.keep_stats, e.gaussians) == (1, 0)
    hpp = open(os.path.join(ROOT, "g2o_frontend_amd", "host", "pwn_hip.hpp")).read()
    for needle in ("pwn_hip_convert_batch_ex", "bool sceneReady = false", "setKeepStats", "bool keepStats = false, bool gaussians = false"):
        assert needle in hpp, needle
    assert os.path.exists(os.path.join(ROOT, "tools", "pwn_hip_scene_ready_check.cpp"))
