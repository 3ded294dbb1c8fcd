#!/usr/bin/env python3
"""Refresh tests/golden/png_batch_files.json: hash the files of its case list with the in-tree
library (or OMR_LIB) and store the sha256.  Needs the GPU.  Run it only for a change that alters
the coded PNG bytes on purpose, and say so in that change.

  python3 tools/png_golden.py [out.json]      (default: rewrite the golden in place)"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "omero-ms-image-region_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import omr
    from test_png_batch_gpu import GOLDEN_FILES, pinned_files_digest
    with open(GOLDEN_FILES) as f:
        golden = json.load(f)
    with omr.Context(0) as ctx:
        golden["sha256"] = pinned_files_digest(ctx, golden["cases"])
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN_FILES, "w") as f:
        json.dump(golden, f, indent=1)
        f.write("\n")
    print(golden["sha256"])


if __name__ == "__main__":
    main()
