"""The stand-in declarations under tests/stubs (Eigen, opencv2) with which tools/check_binding_syntax.py puts the reference-side binding
(bindings/pwn_hip/*.cpp) through `g++ -fsyntax-only` against the reference's own headers.  That pass needs a checkout of the reference,
whose headers cannot be stored here, so it is a tool; what it relies on in this repository is checked here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stand_ins_stay_declarations_only():
    """the stand-ins must never grow into an implementation: no function body beyond empty braces, under 300 lines in all"""
    total = 0
    for dirpath, _, files in os.walk(os.path.join(ROOT, "tests", "stubs")):
        for f in files:
            text = open(os.path.join(dirpath, f)).read()
            total += text.count("\n")
            code = re.sub(r"//[^\n]*", "", text)
            for body in re.findall(r"\)\s*(?:const)?\s*\{([^{}]*)\}", code):
                assert body.strip() == "", (f, body.strip()[:60])
    assert total <= 300, total
