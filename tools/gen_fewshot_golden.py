"""Writes the two fixtures of the few-shot host tests from a checkout of the reference:

  tests/golden/reference_fewshot_cli_tables.json   the argparse tables (flag -> default / action / choices, as source text) of the reference's four
                                                   few-shot entry points, in the format of tests/golden/reference_cls_cli_tables.json
  tests/golden/fewshot_samples.json                name lists returned by the reference's own FewShotDataModule._sample_training_data for recorded
                                                   inputs (names, labels, seed, strategy), classification and segmentation

Only tables and recorded lists are stored, never source text.  The reference's dataset modules import torchvision for their image I/O; the two
few-shot modules are loaded by path inside a throw-away package whose `.classification` / `.segmentation` hold a stub USDataset, and the sampler is
called on an instance made without __init__ (which would read the data directory).  Each case seeds the global `random` as the reference's main does.

    python tools/gen_fewshot_golden.py REFERENCE_DIR
"""
import importlib.util
import json
import os
import random
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_host_fixtures import argparse_table  # noqa: E402

ENTRIES = ["biomedclip/fewshot_classification.py", "biomedclip/fewshot_segmentation.py", "baselines/fewshot_classification.py",
           "baselines/fewshot_segmentation.py"]
SEEDS = (1, 2)
RATIOS = (0.01, 0.1, 1.0)
SHOTS = (1, 2, 100)


def load_sampler(reference_dir, task):
    pkg = types.ModuleType("_ref_datasets")
    pkg.__path__ = []
    sys.modules["_ref_datasets"] = pkg
    stub = types.ModuleType(f"_ref_datasets.{task}")
    stub.USDataset = object
    sys.modules[f"_ref_datasets.{task}"] = stub
    spec = importlib.util.spec_from_file_location(f"_ref_datasets.fewshot_{task}", os.path.join(reference_dir, "src/datasets", f"fewshot_{task}.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.FewShotDataModule


def names_and_labels():
    """40 names, 16 of class 1 and 24 of class 0, interleaved so that class 1 is seen first; and 250 names (class i % 3 != 0) for the 1 % ratio."""
    small = [f"img_{i:03d}.png" for i in range(40)]
    small_labels = [1 if i % 5 in (0, 2) else 0 for i in range(40)]
    assert sum(small_labels) == 16 and small_labels[0] == 1
    large = [f"scan_{i:04d}.png" for i in range(250)]
    large_labels = [int(i % 3 != 0) for i in range(250)]
    return {"small": (small, small_labels), "large": (large, large_labels)}


def main(reference_dir):
    tables = {e: argparse_table(os.path.join(reference_dir, "src/models", e)) for e in ENTRIES}
    out = os.path.join(ROOT, "tests/golden/reference_fewshot_cli_tables.json")
    with open(out, "w") as f:
        json.dump(tables, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {', '.join(f'{e} ({len(t)} flags)' for e, t in tables.items())}")

    Cls, Seg = load_sampler(reference_dir, "classification"), load_sampler(reference_dir, "segmentation")
    sets = names_and_labels()
    cases = []

    def record(task, cls, which, seed, **kw):
        names, labels = sets[which]
        dm = cls.__new__(cls)
        dm.train_ratio, dm.shots_per_class, dm.stratified = kw.get("train_ratio"), kw.get("shots_per_class"), kw.get("stratified", True)
        dm.label_dict = dict(zip(names, labels))
        random.seed(seed)
        sampled = dm._sample_training_data(list(names))
        cases.append(dict(task=task, set=which, seed=seed, sampled=list(sampled), **kw))

    for which in sets:
        for seed in SEEDS:
            for ratio in RATIOS:
                for stratified in (True, False):
                    record("classification", Cls, which, seed, train_ratio=ratio, stratified=stratified)
                record("segmentation", Seg, which, seed, train_ratio=ratio)
            for shots in SHOTS:
                record("classification", Cls, which, seed, shots_per_class=shots, train_ratio=0.1)
    out = os.path.join(ROOT, "tests/golden/fewshot_samples.json")
    with open(out, "w") as f:
        json.dump({"sets": {k: {"names": v[0], "labels": v[1]} for k, v in sets.items()}, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {len(cases)} cases ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1])
