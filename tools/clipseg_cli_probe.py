"""The CLIPSeg entry point under measurement knobs that need nothing from inside its loop (hand-run; the entry point itself reads no knob):
    nogc     the cyclic garbage collector off
    switch   the interpreter's thread switch interval at 50 ms
    power    board power / shader clock sampled from the model's preparation to the end of train() (uia_hip.telemetry: amdgpu hwmon files, no HIP call)

    python tools/clipseg_cli_probe.py nogc,switch,power --dataset BUSI --synthetic ... --stats_json s.json

Runs src/models/clipseg/segmentation.main on the remaining arguments in this process and prints one last line `PROBE {"knobs": ..., "ms_per_iter": ...,
"power": ...}` (ms per iteration over the epochs after the first).  The sampler starts behind prepare_model, i.e. after the loader workers were forked and
the device was bound, so it changes neither."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(argv):
    knobs = set(filter(None, argv[0].split(","))) if argv else set()
    unknown = knobs - {"nogc", "switch", "power"}
    if not argv or unknown:
        raise SystemExit(f"usage: clipseg_cli_probe.py nogc,switch,power|'' [entry point flags]  (unknown: {sorted(unknown)})")
    if "nogc" in knobs:
        import gc
        gc.disable()
    if "switch" in knobs:
        sys.setswitchinterval(0.05)
    import torch
    from src.models import supervised
    from src.models.clipseg import segmentation
    probe = {"knobs": sorted(knobs), "power": None}
    if "power" in knobs:
        from uia_hip.telemetry import PowerSampler
        real_train = supervised.train

        def train(args, task, prepare, forward_kwargs=None):
            sampler = []

            def prepare_then_sample(a):
                model = prepare(a)
                sampler.append(PowerSampler(torch, torch.device(a.device)))
                sampler[0].start()
                return model
            try:
                return real_train(args, task, prepare_then_sample, forward_kwargs)
            finally:
                if sampler:
                    probe["power"] = sampler[0].stop()
        supervised.train = train
    out = segmentation.main(argv[1:])
    steady = out.get("train", {}).get("epochs", [])[1:]
    if steady:
        probe["ms_per_iter"] = round(sum(e["ms"] for e in steady) / max(1, sum(e["updates"] for e in steady)), 3)
    print("PROBE " + json.dumps(probe))


if __name__ == "__main__":
    main(sys.argv[1:])
