"""The ring of byte slots of src/datasets/captions.py with loader workers and no GPU: the checks of tests/test_captions_host.py that fork worker
processes, as functions (called in-process with 0 workers) and as a program (`python caption_ring_driver.py slot|abandon ROOT TOKENIZER WORKERS`, a
fresh process that never opens the GPU)."""
import os
import queue
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def module(root, tokenizer, workers, batch_size=4, img_size=32, context=12):
    from src.datasets import captions as C
    from src.utils.tokenizer_file import FileTokenizer
    args = SimpleNamespace(finetune_root=root, data_pt=None, synthetic=False, img_size=img_size, batch_size=batch_size, num_workers=workers, seed=3)
    return C.DataModule(args, tokenizer=FileTokenizer(tokenizer, context))


def free_slots(ring):
    got = []
    while True:
        try:
            got.append(ring.free.get(timeout=0.3))
        except queue.Empty:
            break
    for s in got:
        ring.free.put(s)
    return sorted(got)


def slot(root, tokenizer, workers):
    """A slot written by a worker's collate holds what folder.pack_ragged gives for the same samples, with the channel count in word 3."""
    from src.datasets import captions as C
    from src.datasets.folder import pack_ragged
    dm = module(root, tokenizer, workers)
    loader = dm.val_dataloader()                                # in order: 3 samples, one partial batch
    ring = loader.collate_fn
    assert loader.num_workers == workers and ring.slots == C.ring_slots(workers) and ring.data.shape[1] == 4 * C.image_limit(32)
    try:
        got = list(loader)
        assert len(got) == 1 and got[0][0] == ring.MARK
        _, s, B, nbytes, texts = got[0]
        samples = [dm.val[i] for i in range(3)]
        buf, desc = pack_ragged([(px, None, geom) for px, geom, _ in samples])
        assert B == 3 and nbytes == buf.numel() and torch.equal(ring.data[s, :nbytes], buf)
        want = desc.clone()
        want[:, 3] = torch.tensor([1 if px.ndim == 2 else 3 for px, _, _ in samples], dtype=torch.int32)
        assert torch.equal(ring.desc[s, :3], want)
        assert list(texts) == [x[2] for x in samples] and torch.equal(ring.ids[s, :3], dm.tokenizer(list(texts)))
        ring.release(s)
        assert free_slots(ring) == list(range(ring.slots))
    finally:
        dm.shutdown()


def abandon(root, tokenizer, workers):
    """More abandoned iterations than there are slots: each takes one batch, leaves the rest (two per worker are in flight) and drains."""
    dm = module(root, tokenizer, workers, batch_size=2)
    loader = dm.train_dataloader()                              # 21 samples: 10 batches
    ring = loader.collate_fn
    dm.start_workers()
    try:
        for epoch in range(ring.slots + 3):
            dm.set_epoch(epoch)
            it = loader.__dict__.pop("_uia_first_iter", None) or iter(loader)
            first = next(it)
            ring.release(first[1])
            ring.drain(loader, it)
        assert free_slots(ring) == list(range(ring.slots))
        n = 0
        for item in loader:                                      # and a whole epoch still runs (more batches than slots: each goes back at once)
            ring.release(item[1])
            n += 1
        assert n == len(loader) == 10
    finally:
        dm.shutdown()


if __name__ == "__main__":
    {"slot": slot, "abandon": abandon}[sys.argv[1]](sys.argv[2], sys.argv[3], int(sys.argv[4]))
    print("ring ok")
