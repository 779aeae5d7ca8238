"""Fresh-process halves of tests/test_captions_gpu.py: loader workers are forked before the process opens the GPU, so these cannot run inside the
pytest process.

    python caption_gpu_driver.py loader ROOT TOKENIZER WORKERS     loader -> prefetcher -> stage against Pillow, bit for bit; prints "loader ok"
    python caption_gpu_driver.py entry FAMILY ARGV...              the family's finetune.main(ARGV); prints its result as one JSON line
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def loader(root, tokenizer, workers, S=32, batch=5):
    import torch
    import caption_ring_driver as R
    import caption_tree as T
    from src.datasets import captions as C
    dm = R.module(root, tokenizer, workers, batch_size=batch, img_size=S)
    train, val = dm.train_dataloader(), dm.val_dataloader()
    assert train.num_workers == workers and val.num_workers == min(workers, 2) and not torch.cuda.is_initialized()
    dm.start_workers()                                          # forked here, before the GPU is touched
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    stage = C.RgbResizeStage(S)
    pfs = {"train": C.CaptionPrefetcher(train, device), "val": C.CaptionPrefetcher(val, device)}
    seen_modes, seen_big, pinned = set(), False, None
    try:
        for name, ds, ld in (("train", dm.train, train), ("val", dm.val, val)):
            for epoch in range(2 if name == "train" else 1):
                dm.set_epoch(epoch)
                order = ld.batch_sampler.sampler.indices()
                n = 0
                for k, (batch_k, tokens, ready) in enumerate(pfs[name]):
                    idx = order[k * batch:(k + 1) * batch]
                    torch.cuda.current_stream().wait_event(ready)
                    images = stage(batch_k)
                    paths, texts = [ds.pairs[i][1] for i in idx], [ds.pairs[i][0] for i in idx]
                    want = T.pillow_batch(paths, S)
                    got = images.cpu()
                    assert got.shape == want.shape and torch.equal(got, want), f"{name} batch {k}: {int((got != want).sum())} values differ from Pillow"
                    assert torch.equal(tokens.cpu(), dm.tokenizer(texts)), f"{name} batch {k}: token ids"
                    seen_big |= any(p.endswith(T.BIG) for p in paths)
                    n += 1
                assert n == len(ld) == (4 if name == "train" else 1)
        assert len(dm.val) == 3                                 # the validation batch is the partial one
        # iterations abandoned after one batch, more often than there are slots: every slot comes back
        ring = train.collate_fn
        for epoch in range(ring.slots + 2):
            dm.set_epoch(epoch)
            for batch_k, tokens, ready in pfs["train"]:
                torch.cuda.current_stream().wait_event(ready)
                stage(batch_k)
                break
            pfs["train"].close()
        torch.cuda.synchronize()
        pinned = ring.pinned
        assert R.free_slots(ring) == list(range(ring.slots))
        from PIL import Image
        for caption, path in dm.train.pairs + dm.val.pairs:
            seen_modes.add(Image.open(path).mode)
        assert {"L", "RGB", "P", "RGBA"} <= seen_modes and len(dm.train.pairs + dm.val.pairs) == T.N_VALID
        assert seen_big, "the file above the per-image limit was in no compared batch"
    finally:
        for pf in pfs.values():
            pf.close()
        dm.shutdown()
    print(f"loader ok (ring registered as pinned memory: {pinned})")


def entry(family, argv):
    import importlib
    out = importlib.import_module(f"src.models.{family}.finetune").main(argv)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    if sys.argv[1] == "loader":
        loader(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        entry(sys.argv[2], sys.argv[3:])
