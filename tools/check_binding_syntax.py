#!/usr/bin/env python3
"""The reference-side binding (bindings/pwn_hip/*.cpp: HipAligner : Aligner, HipDepthImageConverter : DepthImageConverterIntegralImage,
the Cloud* -> device-cloud registry) meets a compiler: `g++ -std=gnu++98 -fsyntax-only` against the reference's OWN headers in a checkout
of the reference (pwn_core/aligner.h:308, depthimageconverter.h:47, cloud.h, ...), with ~200 lines of stand-in DECLARATIONS for the two
libraries it needs and this image lacks (tests/stubs/Eigen, tests/stubs/opencv2: no function has a body, every Eigen expression has one
loose type).  The reference's headers cannot be stored in this repository, so this is a tool run against a checkout, not a test.

What this checks: every reference class, member, accessor, virtual signature, access level and constness the binding relies on, every
call into include/pwn_hip.h, and C++ syntax (it found a most-vexing-parse in hipaligner.cpp that the name checker could not see); and that
the pass is not vacuous (a member the reference does not declare, a protected member reached from outside, a wrong argument count of a
C-ABI call and a write through a const reference are all caught).
What it does NOT check: anything about Eigen / OpenCV semantics -- the stand-ins accept any matrix expression.  It produces no object
code, is not a build of the reference, is not parity evidence and has nothing to do with the oracle.

The reference's own headers carry two diagnostics under a current g++ (an uninstantiated member template of InformationMatrix:
`other.block<3,3>(0,0)` without `.template`, and `return *this` from a const method -- informationmatrix.h:79,81; compilers of the
reference's time did not look into uninstantiated templates).  They are listed below and tolerated; anything else fails.

  tools/check_binding_syntax.py <reference tree>        exit 0: clean, 1: a finding, 2: no reference headers / no g++"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN_REFERENCE_DIAGNOSTICS = {("g2o_frontend/pwn_core/informationmatrix.h", 79), ("g2o_frontend/pwn_core/informationmatrix.h", 81)}
SOURCES = ["devicecloudregistry.cpp", "hipdepthimageconverter.cpp", "hipaligner.cpp"]
NOT_VACUOUS = {
    "no_member": '#include "hipaligner.h"\nvoid f(pwn::HipAligner& a) { a.setOuterIterationz(3); }\n',
    "protected": '#include "hipaligner.h"\nint f(pwn::HipAligner& a) { return a._outerIterations; }\n',
    "capi_args": '#include "pwn_hip.h"\nint f(pwn_hip_ctx* c) { return pwn_hip_ctx_set_subbatch(c, 1); }\n',
    "const": '#include "g2o_frontend/pwn_core/cloud.h"\nvoid f(const pwn::Cloud& c) { c.points().clear(); }\n',
}
OK_SOURCE = '#include "hipaligner.h"\n#include "hipdepthimageconverter.h"\nvoid f(pwn::HipAligner& a) { a.setOuterIterations(3); a.align(); }\n'


def syntax_pass(ref, path):
    cmd = ["g++", "-std=gnu++98", "-fsyntax-only", "-Wall", "-Woverloaded-virtual", "-Wno-unused", "-Wno-deprecated",
           "-I", os.path.join(ROOT, "tests", "stubs"), "-I", ref, "-I", os.path.join(ref, "g2o_frontend", "basemath"),
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bindings", "pwn_hip"), path]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    diags = []
    for line in out.stderr.splitlines():
        m = re.match(r"(.+?):(\d+):(\d+): (error|warning): (.*)", line)
        if m:
            diags.append((m.group(1), int(m.group(2)), m.group(4), m.group(5)))
    return out.returncode, diags


def check(ref):
    """list of findings (empty: clean)"""
    ref = os.path.abspath(ref)
    findings = []
    for src in SOURCES:
        rc, diags = syntax_pass(ref, os.path.join(ROOT, "bindings", "pwn_hip", src))
        ours = [d for d in diags if not d[0].startswith(ref)]
        findings += ["%s: diagnostic in the binding / stand-ins / C-ABI header: %s" % (src, d) for d in ours]
        theirs = {(os.path.relpath(d[0], ref), d[1]) for d in diags if d[0].startswith(ref) and d[2] == "error"}
        findings += ["%s: new diagnostic inside the reference's headers: %s" % (src, d) for d in sorted(theirs - KNOWN_REFERENCE_DIAGNOSTICS)]
        if rc != 0 and not ours and not theirs:
            findings.append("%s: the compiler failed without a located diagnostic" % src)
    with tempfile.TemporaryDirectory() as d:
        for name, code in NOT_VACUOUS.items():
            p = os.path.join(d, name + ".cpp")
            open(p, "w").write(code)
            rc, diags = syntax_pass(ref, p)
            if rc == 0 or not [x for x in diags if x[0] == p and x[2] == "error"]:
                findings.append("vacuous pass: %s was not caught (%s)" % (name, diags[:3]))
        p = os.path.join(d, "ok.cpp")
        open(p, "w").write(OK_SOURCE)
        rc, diags = syntax_pass(ref, p)
        findings += ["a correct use was refused: %s" % (x,) for x in diags if x[0] == p]
    return findings


def main():
    if len(sys.argv) != 2:
        print(__doc__.strip().splitlines()[-1]); return 2
    ref = sys.argv[1]
    if not os.path.isdir(os.path.join(ref, "g2o_frontend", "pwn_core")) or shutil.which("g++") is None:
        print("needs the reference headers under", os.path.join(ref, "g2o_frontend", "pwn_core"), "and g++"); return 2
    findings = check(ref)
    for f in findings:
        print(f)
    print("binding syntax check: %d sources + %d non-vacuity cases, %d findings" % (len(SOURCES), len(NOT_VACUOUS) + 1, len(findings)))
    return 1 if findings else 0


if __name__ == "__main__":
    sys.exit(main())
