"""Regenerates tests/golden/reference_lines.json: the name and line count of every C# / HLSL / shader file of the reference
(aras-p/UnityGaussianSplatting), which tests/test_citations.py holds every `File.ext:line` citation of this repository against.

    python tests/golden/make_reference_lines.py <reference checkout>

Where a name occurs more than once the largest line count is kept (a citation names a file, not a path)."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
EXT = re.compile(r"\.(?:cs|hlsl|compute|shader|cginc)$")


def main(ref: str) -> None:
    if not os.path.isdir(os.path.join(ref, "package")):
        raise SystemExit(f"{ref}: not a checkout of the reference (no package/)")
    lines = {}
    for dp, _, fs in os.walk(ref):
        for f in fs:
            if EXT.search(f):
                with open(os.path.join(dp, f), errors="replace") as fh:
                    lines[f] = max(lines.get(f, 0), sum(1 for _ in fh))
    with open(os.path.join(HERE, "reference_lines.json"), "w") as fh:
        json.dump({"reference": "aras-p/UnityGaussianSplatting", "lines": dict(sorted(lines.items()))}, fh, indent=1)
        fh.write("\n")
    print(f"{len(lines)} files")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
