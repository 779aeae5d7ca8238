"""Writes the ResNet-baseline fixtures under tests/golden/:

    reference_baseline_cls_cli_table.json   the argparse table of the reference's src/models/baselines/classification.py (flag -> default / action /
                                            choices, as oracle.gen_host_fixtures.argparse_table reads them: tables only, no source text)
    resnet18_keys.json                      the state-dict names and shapes of torchvision's resnet18() at 1000 classes, in its order

The names come from an installed torchvision when there is one; otherwise from tests/resnet_reference.state_shapes, which restates
torchvision's documented structure (the file then says so in its "source" field).  With torchvision present the two are compared.

    python tools/gen_resnet_baseline_golden.py REFERENCE_DIR
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.gen_host_fixtures import argparse_table  # noqa: E402

import resnet_reference as RR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main(reference_dir):
    table = argparse_table(os.path.join(reference_dir, "src/models/baselines/classification.py"))
    with open(os.path.join(GOLDEN, "reference_baseline_cls_cli_table.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    restated = [[k, list(s)] for k, s in RR.state_shapes("resnet18", 1000)]
    try:
        from torchvision import models
        state = [[k, list(v.shape)] for k, v in models.resnet18().state_dict().items()]
        assert state == restated, "the restated structure differs from the installed torchvision's"
        source = "torchvision.models.resnet18().state_dict()"
    except ImportError:
        state, source = restated, "torchvision's documented structure, restated in tests/resnet_reference.py (no torchvision installed when this was written)"
    with open(os.path.join(GOLDEN, "resnet18_keys.json"), "w") as f:
        json.dump({"source": source, "state": state}, f, indent=0)
        f.write("\n")
    print("wrote", len(table), "flags and", len(state), "state-dict entries")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/gen_resnet_baseline_golden.py REFERENCE_DIR")
    main(sys.argv[1])
