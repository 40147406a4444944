"""Every `File.ext:line[-line]` citation of the reference in the header, the design documents, the kernels, the host layer, the oracle and the tests names a
file of the reference and lines that file has.  The reference's file names and line counts are recorded in tests/golden/reference_lines.json
(tests/golden/make_reference_lines.py), so the test needs no reference checkout."""
import glob
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CITE = re.compile(r"\b([A-Za-z0-9_]+\.(?:cs|hlsl|compute|shader|cginc))[:](\d+)(?:[-–](\d+))?")


def test_reference_citations_point_at_existing_lines():
    with open(os.path.join(ROOT, "tests", "golden", "reference_lines.json")) as f:
        lengths = json.load(f)["lines"]
    files = [os.path.join(ROOT, f) for f in ("include/gsplat_c.h", "DESIGN.md", "INTEGRATION.md", "README.md", "bench.py", "__graft_entry__.py")]
    for pat in ("unitygaussiansplatting_amd/csrc/*", "unitygaussiansplatting_amd/*.py", "unitygaussiansplatting_amd/dotnet/*.cs", "oracle/*.cpp", "oracle/*.h",
                "oracle/ref_build/*.py", "oracle/ref_build/*.h", "oracle/ref_build/*.cpp", "tests/*.py", "tests/*.c"):
        files += glob.glob(os.path.join(ROOT, pat))
    seen, bad = 0, []
    for fn in files:
        if not os.path.isfile(fn):
            continue
        for m in CITE.finditer(open(fn, errors="replace").read()):
            name, a, b = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
            seen += 1
            if name not in lengths:
                bad.append((os.path.relpath(fn, ROOT), m.group(0), "no such file in the reference")); continue
            if not (1 <= a <= b <= lengths[name]):
                bad.append((os.path.relpath(fn, ROOT), m.group(0), f"the file has {lengths[name]} lines"))
    assert seen > 200, seen
    assert not bad, bad
