"""Writes tests/golden/reference_cli_retrieval.json: the argparse table (flag -> default / action / choices, as source text) of the reference's
retrieval entry point, in the format of tests/golden/reference_cli_tables.json.  Only the table is stored, never source text.

    python tools/gen_retrieval_cli_table.py REFERENCE_DIR
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_host_fixtures import argparse_table  # noqa: E402

ENTRY = "biomedclip/retrieval.py"


def main(reference_dir):
    table = {ENTRY: argparse_table(os.path.join(reference_dir, "src/models", ENTRY))}
    out = os.path.join(ROOT, "tests/golden/reference_cli_retrieval.json")
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {ENTRY} ({len(table[ENTRY])} flags)")


if __name__ == "__main__":
    main(sys.argv[1])
