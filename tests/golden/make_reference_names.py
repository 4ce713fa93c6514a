#!/usr/bin/env python3
"""Extracts the names the reference's headers declare into tests/golden/reference_names.json, so that the name checks of the binding and of
the host mirrors run without the reference tree:

  * "inline_accessors": per header, the public names of its `inline` members (what tests/test_mirror_names.py requires the mirrors to carry);
  * "binding_check": every `_name` word and every word followed by `(` of the headers the binding includes (tools/check_binding_names.py).

Only identifiers are stored, no code.  usage: python tests/golden/make_reference_names.py <reference tree>"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_binding_names  # noqa: E402

INLINE_HEADERS = {"pwn_core": ["aligner.h", "correspondencefinder.h", "linearizer.h", "depthimageconverter.h", "statscalculatorintegralimage.h",
                               "informationmatrixcalculator.h", "pinholepointprojector.h", "pointprojector.h", "cloud.h", "merger.h", "voxelcalculator.h"],
                  "pwn_tracker": ["pwn_matcher_base.h", "pwn_tracker.h"]}


def inline_names(path):
    text = open(path).read()
    names = set()
    for m in re.finditer(r"inline\s+[^;{(]*?[\s&*]([A-Za-z]\w*)\s*\(", text):
        n = m.group(1)
        if not n.startswith("_") and n != "operator":
            names.add(n)
    return sorted(names)


if __name__ == "__main__":
    ref = sys.argv[1]
    d = {"inline_accessors": {h: inline_names(os.path.join(ref, "g2o_frontend", sub, h)) for sub, hs in INLINE_HEADERS.items() for h in hs},
         "binding_check": check_binding_names.reference_names(ref)}
    json.dump(d, open(os.path.join(HERE, "reference_names.json"), "w"), indent=1, sort_keys=True)
    print({k: len(v) for k, v in d.items()}, {k: len(v) for k, v in d["binding_check"].items()})
