"""BiomedCLIP supervised classification with the feature-pyramid adapter on the HIP path — counterpart of the reference's
src/models/biomedclip/classification.py, and the loop the clip / metaclip / unimedclip classification entry points run with their own flags and model.

Kept: the command line (:29-73; default --mona_variant hybrid, batch 32, 200 epochs, AdamW betas 0.9/0.95), model assembly (:80-150: optional LoRA or Mona
adapters loaded BY NAME from a fine-tune checkpoint, TimmCLIPAdapter(task="cls") on layers 3/6/9, freeze_clip_backbone()), the loop (:153-284):
FocalLoss(to_onehot_y=True) per iteration, AdamW with a per-iteration cosine schedule, validation at `epoch > 0 and epoch % 10 == 0` and at the last epoch,
the best-by-accuracy (strict >) checkpoint {"reduces", "blocks", "cls_head", "mona"}, early stopping by --patience and the test-split pass after every
validation; `test()` (:287-365: checkpoint -> heads + Mona parameters by name -> metrics over the test split -> the Acc / Rec / Pre / F1 / AUC table,
results.csv and the <time>_acc=XX.XX backup folder) and `main` (train unless --test, then ALWAYS test).
Different on purpose: the iteration is engine.segmentation_step (zero_grad -> forward -> criterion -> backward -> AdamW, nothing read on the host) with the
focal loss on the device (src/losses/focal.py); batches through engine.DevicePrefetcher; --strong_augs / --weak_augs applied to --data_pt training batches on
the device (src/datasets/augment.py); the metrics on the device (src/utils/cls_metrics.py, one host read
per split).  ROC plots and TensorBoard figures are out of scope; scalars go to <train dir>/log/scalars.jsonl.  Data: `--synthetic` or `--data_pt`
(src/datasets/classification.py).
"""
import argparse
import logging
import os
import random
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import numpy as np
import torch

from src.adapters import inject_lora_to_biomedclip, inject_mona_variant_to_open_clip
from src.datasets import classification as dataset_cls
from src.datasets.augment import stage_for
from src.losses.focal import FocalLoss
from src.models.biomedclip.zero_shot import load_adapter_by_name
from src.third_party.biomedclip.model import create_biomedclip
from src.third_party.timm.clip_adapter import TimmCLIPAdapter
from src.utils.cls_metrics import ClassificationMetrics, report_cls_test
from src.utils.tools import ScalarLog, default_device, fresh_viz_dir, model_summary, parse_config, setup_logging
from uia_hip import functional as UF
from uia_hip.engine import DevicePrefetcher, FlatAdapterOptimizer, cosine_lr, segmentation_step


def add_build_args(p, synthetic_train=256):
    """The additions of this build shared by the four classification entry points (beside the reference's flags)."""
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--synthetic_train", type=int, default=synthetic_train)
    p.add_argument("--synthetic_val", type=int, default=64)
    p.add_argument("--synthetic_test", type=int, default=64)
    p.add_argument("--stats_json", type=str, default=None)
    p.add_argument("--data_pt", type=str, default=None)
    p.add_argument("--ckpt_path", type=str, default=None, help="backbone state dict (.pt); random init if absent")
    p.add_argument("--model_config", type=str, default=None)
    p.add_argument("--extract_layers", type=str, default="3,6,9", help="transformer blocks tapped by the adapter (reference: fixed 3,6,9)")
    p.add_argument("--val_every", type=int, default=10, help="epochs between validations (reference: fixed 10)")


def get_args(argv=None):
    p = argparse.ArgumentParser("Adaptation of Visual Foundation Model for Medical Ultrasound Image Analysis")
    p.add_argument("--exp", type=str, default="biomedclip_cls")
    p.add_argument("--dataset", type=str, default="LN-INT")
    p.add_argument("--img_size", type=int, default=224)
    p.add_argument("--patch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=True, action=argparse.BooleanOptionalAction)
    p.add_argument("--weak_augs", default=True, action=argparse.BooleanOptionalAction)
    p.add_argument("--mona_variant", type=str, default="hybrid")
    p.add_argument("--mona_weights", type=str, default=None)
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--reduce_dim", type=int, default=512)
    p.add_argument("--mona_bottleneck", type=int, default=64)
    p.add_argument("--mona_layers", type=int, default=None)
    p.add_argument("--lora_weights", type=str, default=None)
    p.add_argument("--lora_r", type=int, default=16)
    p.add_argument("--lora_alpha", type=int, default=32)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--epochs", type=int, default=200)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--lr_min", type=float, default=1e-8)
    p.add_argument("--weight_decay", type=float, default=0.01)
    p.add_argument("--beta1", type=float, default=0.9)
    p.add_argument("--beta2", type=float, default=0.95)
    p.add_argument("--device", type=str, default=default_device())
    p.add_argument("--patience", type=int, default=15)
    p.add_argument("--test", default=False, action="store_true")
    add_build_args(p)
    return p.parse_args(argv)


criterion = FocalLoss(to_onehot_y=True)                         # reference :77


def extract_layers(args):
    return [int(v) for v in args.extract_layers.split(",")]


def prepare_model(args):
    cfg = parse_config(args.model_config) if args.model_config else None
    state = torch.load(args.ckpt_path, map_location="cpu") if args.ckpt_path else None
    clip_model = create_biomedclip(state_dict=state, config=cfg, seed=args.seed)
    clip_model.float()
    if args.lora_weights:
        inject_lora_to_biomedclip(clip_model, lora_r=args.lora_r, lora_alpha=args.lora_alpha, lora_dropout=0.0)
        n = load_adapter_by_name(clip_model, args.lora_weights, "lora_state_dict")
        logging.info(f"✓ Loaded {n} pretrained LoRA parameters from {args.lora_weights}")
    elif args.mona_weights:
        inject_mona_variant_to_open_clip(clip_model, variant=args.mona_variant, bottleneck_dim=args.mona_bottleneck, num_layers=args.mona_layers)
        n = load_adapter_by_name(clip_model, args.mona_weights, "mona_state_dict")
        logging.info(f"✓ Loaded {n} pretrained MONA parameters from {args.mona_weights}")
    adapter = TimmCLIPAdapter(clip_model=clip_model, extract_layers=extract_layers(args), reduce_dim=args.reduce_dim, num_classes=args.num_classes,
                              img_size=args.img_size, patch_size=args.patch_size, task="cls")
    adapter.to(args.device)
    adapter.freeze_clip_backbone()
    return adapter


def checkpoint_dict(model):
    """reference :236-246: adapter heads as module state dicts plus the backbone's Mona parameters by full name.  A model with its own
    `checkpoint_dict()` (the DINOv2 classifier: the head's state dict alone) saves that instead."""
    if hasattr(model, "checkpoint_dict"):
        return model.checkpoint_dict()
    return {"reduces": model.reduces.state_dict(), "blocks": model.blocks.state_dict(), "cls_head": model.cls_head.state_dict(),
            "mona": {n: p.data.clone() for n, p in model.named_parameters() if "mona" in n}}


def evaluate(model, loader_pf, accumulator):
    cur = torch.cuda.current_stream()
    with torch.no_grad():
        for images, labels, ready in loader_pf:
            cur.wait_event(ready)
            accumulator.update(model(images.float()).detach(), labels.detach())


def _log_stats(writer, args, split, stats, iter_num):
    for k in ("loss", "acc", "pre", "rec", "f1", "auc"):
        writer.add_scalar(f"{args.exp}/{split}_{k}", stats[k], iter_num)
    writer.flush()


def train(args, prepare=None):
    """prepare: another family's `prepare_model(args) -> adapter` around the same loop (reference :153-284)."""
    if not torch.cuda.is_initialized():
        torch.set_num_threads(max(1, min(4, torch.get_num_threads())))
    dm = dataset_cls.DataModule(args)
    trainloader, valloader, testloader = dm.train_dataloader(), dm.val_dataloader(), dm.test_dataloader()
    torch.cuda.set_device(torch.device(args.device))
    UF.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    UF.set_dropout_seed(args.seed)
    model = (prepare or prepare_model)(args)
    model.train()
    logging.info(model_summary({"model": model}))
    writer = ScalarLog(args.train_snapshot_path + "/log")
    logging.info("Start training")
    opt = FlatAdapterOptimizer([(n, p) for n, p in model.named_parameters() if p.requires_grad], lr=args.lr, betas=(args.beta1, args.beta2),
                               weight_decay=args.weight_decay, max_norm=0.0)
    max_iters = len(trainloader) * args.epochs
    train_pf = DevicePrefetcher(trainloader, None, args.device, second=dataset_cls.second_of)
    val_pf = DevicePrefetcher(valloader, None, args.device, second=dataset_cls.second_of)
    test_pf = DevicePrefetcher(testloader, None, args.device, second=dataset_cls.second_of)
    iter_num, best_val_acc, patience, logged, last = 0, 0.0, 0, [], None
    epoch_ms, val_hist = [], []
    cur = torch.cuda.current_stream()
    augment = stage_for(args, with_mask=False)                   # --strong_augs / --weak_augs on --data_pt batches; None: bypassed
    for epoch in range(args.epochs):
        torch.cuda.synchronize()
        t0, n_it = time.perf_counter(), 0
        if augment is not None:
            augment.set_epoch(epoch)
        for images, labels, ready in train_pf:
            cur.wait_event(ready)
            if augment is not None:
                images, _ = augment(images)
            loss, _ = segmentation_step(model, criterion, opt, images.float(), labels, lr=cosine_lr(args.lr, args.lr_min, iter_num, max_iters))
            if iter_num % 10 == 0:
                logged.append((iter_num, loss))
            iter_num += 1
            n_it += 1
        torch.cuda.synchronize()
        epoch_ms.append({"ms": (time.perf_counter() - t0) * 1e3, "updates": n_it})
        if not ((epoch > 0 and epoch % args.val_every == 0) or (epoch == args.epochs - 1)):
            continue
        model.eval()
        for it, l in logged:
            writer.add_scalar(f"{args.exp}/train_loss", l, it)
        last = float(logged[-1][1]) if logged else last
        logged = []
        accumulator = ClassificationMetrics(criterion=criterion, num_classes=args.num_classes)
        evaluate(model, val_pf, accumulator)
        stats = accumulator.compute()
        accumulator.reset()
        _log_stats(writer, args, "val", stats, iter_num)
        val_hist.append({"epoch": epoch, **stats})
        if stats["acc"] > best_val_acc:
            patience, best_val_acc = 0, stats["acc"]
            torch.save(checkpoint_dict(model), os.path.join(args.train_snapshot_path, "best_model.pth"))
        else:
            patience += 1
        if patience >= args.patience:
            logging.info(f"\nEarly stopping at epoch {epoch + 1}")
            break
        logging.info(f"\titer: {iter_num}, loss: {stats['loss']:.4f}, acc: {stats['acc'] * 100:.2f}, rec: {stats['rec'] * 100:.2f}, "
                     f"pre: {stats['pre'] * 100:.2f}, f1: {stats['f1'] * 100:.2f}, auc: {stats['auc'] * 100:.2f}")
        evaluate(model, test_pf, accumulator)                   # reference :260-278
        tstats = accumulator.compute()
        accumulator.reset()
        _log_stats(writer, args, "test", tstats, iter_num)
        val_hist[-1]["test"] = tstats
        model.train()
    writer.close()
    for pf in (train_pf, val_pf, test_pf):
        pf.close()
    if not os.path.exists(os.path.join(args.train_snapshot_path, "best_model.pth")):
        logging.warning("no validation improved on an accuracy of 0.0: saving the last iterate as best_model.pth (the reference has no checkpoint then and fails in test())")
        torch.save(checkpoint_dict(model), os.path.join(args.train_snapshot_path, "best_model.pth"))
    out = {"iters": iter_num, "best_val_acc": best_val_acc, "last_loss": last, "val": val_hist, "epochs": epoch_ms,
           "augmented_images": augment.augmented if augment is not None else 0}
    if args.stats_json:
        import json
        with open(args.stats_json, "w") as f:
            json.dump(out, f)
    return out


@torch.no_grad()
def test(args, prepare=None):
    """reference :287-365."""
    logging.info("Start testing")
    torch.cuda.set_device(torch.device(args.device))
    UF.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    model = (prepare or prepare_model)(args)
    saved_best = os.path.join(args.train_snapshot_path, "best_model.pth")
    adapter_state_dict = torch.load(saved_best, map_location="cpu")
    if hasattr(model, "load_checkpoint"):                       # the counterpart of a model's own checkpoint_dict()
        model.load_checkpoint(adapter_state_dict)
    else:
        model.reduces.load_state_dict(adapter_state_dict["reduces"])
        model.blocks.load_state_dict(adapter_state_dict["blocks"])
        model.cls_head.load_state_dict(adapter_state_dict["cls_head"])
        mona_state_dict = adapter_state_dict["mona"]
        for name, param in model.named_parameters():            # :301-304 (copy_ instead of re-pointing .data: the T copies of the weights are keyed by version)
            if "mona" in name:
                param.copy_(mona_state_dict[name].to(param.device))
    UF.WEIGHTS.bump()
    model.eval()
    dm = dataset_cls.DataModule(args)
    testloader = dm.test_dataloader()
    fresh_viz_dir(args)
    accumulator = ClassificationMetrics(criterion=criterion, num_classes=args.num_classes)
    test_pf = DevicePrefetcher(testloader, None, args.device, second=dataset_cls.second_of)
    evaluate(model, test_pf, accumulator)
    stats = accumulator.compute()
    accumulator.reset()
    test_pf.close()
    stats["results_csv"] = report_cls_test(args, stats, saved_best)
    return stats


def run(args, prepare=None):
    """main() of every classification entry point: seeds, run directories, train unless --test, then ALWAYS test (reference :368-394)."""
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    args.train_snapshot_path = f"runs/{args.exp}/{args.dataset}/train"
    args.test_snapshot_path = f"runs/{args.exp}/{args.dataset}/test"
    for path in (args.train_snapshot_path, args.test_snapshot_path):
        os.makedirs(path, exist_ok=True)
    out = {}
    if not args.test:
        setup_logging(args, args.train_snapshot_path)
        out = train(args, prepare)
    setup_logging(args, args.test_snapshot_path)
    out["test"] = test(args, prepare)
    return out


def main(argv=None):
    return run(get_args(argv))


if __name__ == "__main__":
    main()
