"""Writes tests/golden/reference_seg_cli_tables.json: the argparse tables (flag -> default / action / choices, as source text) of the reference's three
CLIP-family segmentation entry points, in the format of tests/golden/reference_cli_tables.json.  Only the tables are stored, never source text.

    python tools/gen_seg_cli_tables.py REFERENCE_DIR
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_host_fixtures import argparse_table  # noqa: E402

ENTRIES = ["clip/segmentation.py", "metaclip/segmentation.py", "unimedclip/segmentation.py"]


def main(reference_dir):
    tables = {e: argparse_table(os.path.join(reference_dir, "src/models", e)) for e in ENTRIES}
    out = os.path.join(ROOT, "tests/golden/reference_seg_cli_tables.json")
    with open(out, "w") as f:
        json.dump(tables, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {', '.join(f'{e} ({len(t)} flags)' for e, t in tables.items())}")


if __name__ == "__main__":
    main(sys.argv[1])
