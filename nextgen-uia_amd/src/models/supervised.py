"""The supervised training loop of the classification and segmentation entry points: `train`, `test`, `run` (the body of every `main`), the build's
shared flags (`add_build_args`) and the task descriptions the loop reads (`CLASSIFICATION`, `SEGMENTATION`, and their few-shot forms
`FEWSHOT_CLASSIFICATION`, `FEWSHOT_SEGMENTATION`: the reference's src/models/{biomedclip,baselines}/fewshot_*.py — the same loops on a training list
sampled once (src/datasets/fewshot_*.py), whose batches are formed on the device from the resident set (src/datasets/resident.py); one process).

What the reference repeats per family (src/models/*/classification.py, src/models/*/segmentation.py): FocalLoss / DiceCE per iteration, AdamW with a
per-iteration cosine schedule and no clipping, validation at `epoch > 0 and epoch % 10 == 0` and at the last epoch, the best checkpoint by a strict >
on one metric, early stopping by --patience, a test-split pass after every validation; `test()`: best_model.pth -> model -> metrics over the test split ->
the results table, results.csv and the backup folder, and for segmentation the reference's visualize_seg pictures of every test image
(src/utils/viz.py: one launch per batch, written by background threads; --no-viz leaves the folder empty; the test passes inside train() write none); `main`: train unless --test, then ALWAYS test.
Different on purpose: the iteration is engine.segmentation_step (zero_grad -> forward -> criterion -> backward -> AdamW, nothing read on the host; every
tenth loss is kept as a device scalar and written at validation time), batches arrive through engine.DevicePrefetcher, --strong_augs / --weak_augs act
on --data_pt training batches on the device (src/datasets/augment.py), --data_root reads the reference's dataset folders (src/datasets/folder.py: the
workers decode, a ResizeStage ahead of the augmentation makes PIL's resize on the device and yields the --data_pt batch of the same files), metrics are computed on the device (one host read per split), scalars go to
<train dir>/log/scalars.jsonl.  If no validation ever improves on 0.0 the last iterate is saved, so test() has a checkpoint.

What differs by task is a field of `Task`; what differs by model is an argument: `prepare(args) -> model`, and `forward_kwargs(args) -> (batch size ->
dict of extra forward keyword arguments)`, called once behind the model's preparation (CLIPSeg: its prompt).  A model says what its checkpoint holds:
`checkpoint_dict()` and `load_checkpoint(state)`.
"""
import argparse
import dataclasses
import functools
import logging
import os
import random
import time
from dataclasses import dataclass

import numpy as np
import torch

from src.datasets import classification as dataset_cls
from src.datasets import fewshot_classification as dataset_fs_cls
from src.datasets import fewshot_segmentation as dataset_fs_seg
from src.datasets import folder as dataset_folder
from src.datasets import segmentation as dataset_seg
from src.datasets.augment import stage_for
from src.datasets.resident import resident_for
from src.losses.dice import DiceCELoss
from src.losses.focal import FocalLoss
from src.utils.cls_metrics import ClassificationMetrics, report_cls_test
from src.utils.tools import MetricAccumulator, ScalarLog, fresh_viz_dir, model_summary, report_test, setup_logging
from src.utils.viz import SegVisualizer
from uia_hip import functional as UF
from uia_hip.engine import DevicePrefetcher, FlatAdapterOptimizer, bind_device, cosine_lr, dist_env, init_data_parallel, segmentation_step


@dataclass(frozen=True)
class Task:
    data: object                    # the src.datasets module: DataModule, second_of
    criterion: object
    metrics: object                 # (criterion=, num_classes=) -> accumulator with update / compute / reset
    report: object                  # (args, stats, saved_best, rank) -> results.csv path: the tail of test()
    best: str                       # the validation figure that decides "best" (strict >) ...
    best_name: str                  # ... its key in train()'s dict ...
    best_words: str                 # ... and its name in the last-iterate warning
    scalars: tuple                  # figures written per split as <exp>/<split>_<name without _mean>
    line: object                    # stats -> the tail of the one-line log after a validation
    to_input: object                # (images, labels, in_channels, bufs) -> what the model and the criterion take
    with_mask: bool                 # the augmentation stage transforms the second tensor too
    data_parallel: bool             # one process per GPU under torch.distributed.run (rank 0 saves; "rank" / "world" in train()'s dict), loader workers forked before the
                                    # first GPU call, the next epoch's iterator made before validation.  False: this process alone, a fresh iterator per epoch
    val_history: bool               # train()'s dict carries "val": per validation its figures and the test pass's
    lr_scalar: bool = False         # <exp>/lr beside every logged training loss
    loop_timings: bool = False      # epoch records carry loader_wait_ms / enqueue_ms / drain_ms
    stop_twice: bool = False        # the reference's second early-stopping line
    visualize: bool = False         # test() writes the reference's three pictures per test image into <test dir>/viz (src/utils/viz.py) unless --no-viz
    train_module: object = None     # (args, rank=, world=) -> the data module of train(); None: data.DataModule.  test() always uses data.DataModule
    resident: bool = False          # training batches are formed on the device from the module's resident_rows() (src/datasets/resident.py): no training
                                    # loader; the module carries original_train_count / sampled_train_count, which train()'s dict repeats
    roc_csv: bool = False           # after each validation: <train dir>/roc_curves/roc_curve_iter_<iter>.csv (the data of the reference's plot_roc_curve)


def _cls_input(images, labels, in_channels, bufs=None):
    return images.float(), labels


def _cls_line(s):
    return (f"acc: {s['acc'] * 100:.2f}, rec: {s['rec'] * 100:.2f}, pre: {s['pre'] * 100:.2f}, f1: {s['f1'] * 100:.2f}, auc: {s['auc'] * 100:.2f}")


def _seg_metrics(criterion, num_classes):
    return MetricAccumulator(type="seg", criterion=criterion, num_classes=num_classes)


def _seg_line(s):
    return f"dice: {s['dice_mean'] * 100:.2f}, iou: {s['iou_mean'] * 100:.2f}, hd95: {s['hd95_mean']:.2f}, asd: {s['asd_mean']:.2f}"


CLASSIFICATION = Task(data=dataset_cls, criterion=FocalLoss(to_onehot_y=True), metrics=ClassificationMetrics, report=report_cls_test,
                      best="acc", best_name="best_val_acc", best_words="an accuracy", scalars=("loss", "acc", "pre", "rec", "f1", "auc"), line=_cls_line,
                      to_input=_cls_input, with_mask=False, data_parallel=False, val_history=True)
SEGMENTATION = Task(data=dataset_seg, criterion=DiceCELoss(smooth_nr=1e-8, smooth_dr=1e-8), metrics=_seg_metrics, report=report_test, best="dice_mean", best_name="best_val_dice", best_words="a mean Dice", scalars=("loss", "dice_mean", "iou_mean"),
                    line=_seg_line, to_input=functools.partial(dataset_seg.as_model_input, widen=False), with_mask=True, data_parallel=True,
                    val_history=False, visualize=True)
FEWSHOT_CLASSIFICATION = dataclasses.replace(CLASSIFICATION, train_module=dataset_fs_cls.from_args, resident=True, roc_csv=True)
FEWSHOT_SEGMENTATION = dataclasses.replace(SEGMENTATION, train_module=dataset_fs_seg.from_args, resident=True, data_parallel=False)


def add_build_args(p, synthetic_train=256):
    """The additions of this build shared by the entry points (beside the reference's flags)."""
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--synthetic_train", type=int, default=synthetic_train)
    p.add_argument("--synthetic_val", type=int, default=64)
    p.add_argument("--synthetic_test", type=int, default=64)
    p.add_argument("--stats_json", type=str, default=None)
    p.add_argument("--data_pt", type=str, default=None)
    p.add_argument("--data_root", type=str, default=None,
                   help="the reference's dataset folders (<dir>/{classification,segmentation}/<dataset>/*.txt, <dir>/all/{images,masks}); after --data_pt and --synthetic")
    p.add_argument("--ckpt_path", type=str, default=None, help="backbone state dict (.pt); random init if absent")
    p.add_argument("--model_config", type=str, default=None)
    p.add_argument("--extract_layers", type=str, default="3,6,9", help="transformer blocks tapped by the adapter (reference: fixed 3,6,9)")
    p.add_argument("--val_every", type=int, default=10, help="epochs between validations (reference: fixed 10)")
    p.add_argument("--viz", default=True, action=argparse.BooleanOptionalAction,
                   help="segmentation test(): write <stem>.png / <stem>_overlay.png / <stem>_pred.png per test image (reference: always)")


def extract_layers(args):
    return [int(v) for v in args.extract_layers.split(",")]


_NO_KWARGS = {}


def _no_kwargs(n):
    return _NO_KWARGS


def _bind(args, task):
    if task.data_parallel:
        bind_device(args)                                        # cuda:LOCAL_RANK before anything is allocated
    else:
        torch.cuda.set_device(torch.device(args.device))
    UF.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)


def _data_module(args, task, rank, world):
    """task.data.DataModule, or the folder loader's when --data_root is what the DataModules' precedence picks (src/datasets/folder.py)."""
    if dataset_folder.chosen(args):
        return dataset_folder.DataModule(args, "segmentation" if task.with_mask else "classification", rank=rank, world=world)
    return task.data.DataModule(args, rank=rank, world=world)


def _prefetcher(args, task, loader):
    if dataset_folder.chosen(args):
        return dataset_folder.RaggedPrefetcher(loader, args.device)
    return DevicePrefetcher(loader, None, args.device, second=task.data.second_of)


def evaluate(task, model, loader_pf, accumulator, in_channels=3, kwargs_for=_no_kwargs, viz=None, name_of=None, resize=None):
    """One pass of a validation / test split.  viz: a src.utils.viz.SegVisualizer that takes every batch behind its metrics, with name_of(i) the file
    name of sample i of the split (the prefetcher drops names; these loaders do not shuffle, so a running index is the sample's).  resize: the
    src.datasets.folder.ResizeStage of a --data_root run, which turns the prefetcher's ragged batch into the batch everything below takes."""
    cur = torch.cuda.current_stream()
    to_input = task.to_input
    seen = 0
    with torch.no_grad():
        for images, labels, ready in loader_pf:
            cur.wait_event(ready)
            if resize is not None:
                images, labels = resize(images, labels)
            images, labels = to_input(images, labels, in_channels)
            preds = model(images, **kwargs_for(images.shape[0])).detach()
            accumulator.update(preds, labels.detach())
            if viz is not None:
                viz.submit(images, labels, preds, [name_of(seen + j) for j in range(images.shape[0])])
                seen += images.shape[0]


def _write_roc_csv(accumulator, folder, iter_num):
    fpr, tpr, thr = (t.cpu().tolist() for t in accumulator.roc())
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, f"roc_curve_iter_{iter_num}.csv"), "w") as f:
        f.write("fpr,tpr,threshold\n")
        f.writelines(f"{a!r},{b!r},{c!r}\n" for a, b, c in zip(fpr, tpr, thr))


def _split_pass(task, model, loader_pf, accumulator, args, kwargs_for, writer, split, iter_num, roc_dir=None, resize=None):
    evaluate(task, model, loader_pf, accumulator, args.in_channels, kwargs_for, resize=resize)
    stats = accumulator.compute()
    if roc_dir is not None:
        _write_roc_csv(accumulator, roc_dir, iter_num)
    accumulator.reset()
    for k in task.scalars:
        writer.add_scalar(f"{args.exp}/{split}_{k.replace('_mean', '')}", stats[k], iter_num)
    writer.flush()
    return stats


def train(args, task, prepare, forward_kwargs=None):
    rank, _, world = dist_env() if task.data_parallel or task.resident else (0, 0, 1)      # resident: the module refuses a world above 1
    if not torch.cuda.is_initialized():
        torch.set_num_threads(max(1, min(4, torch.get_num_threads())))
    dm = task.train_module(args, rank=rank, world=world) if task.train_module else _data_module(args, task, rank, world)
    if task.resident:
        logging.info(f"Training samples: {dm.sampled_train_count} / {dm.original_train_count}")
    trainloader = None if task.resident else dm.train_dataloader()
    valloader, testloader = dm.val_dataloader(), dm.test_dataloader()
    dm.start_workers()                                           # loader worker processes are forked BEFORE this process touches the GPU
    _bind(args, task)
    UF.set_dropout_seed(args.seed + 7919 * rank)
    model = prepare(args)
    model.train()
    logging.info(model_summary({"model": model}))
    writer = ScalarLog(args.train_snapshot_path + "/log")
    logging.info("Start training")
    kwargs_for = forward_kwargs(args) if forward_kwargs is not None else _no_kwargs
    opt = FlatAdapterOptimizer([(n, p) for n, p in model.named_parameters() if p.requires_grad], lr=args.lr, betas=(args.beta1, args.beta2),
                               weight_decay=args.weight_decay, max_norm=0.0)              # no clipping in these loops
    if world > 1:
        init_data_parallel(opt)
    train_pf = resident_for(args, dm, rank) if task.resident else _prefetcher(args, task, trainloader)
    val_pf, test_pf = (_prefetcher(args, task, loader) for loader in (valloader, testloader))
    max_iters = len(train_pf if task.resident else trainloader) * args.epochs
    best_path = os.path.join(args.train_snapshot_path, "best_model.pth")
    iter_num, best, patience, logged, last = 0, 0.0, 0, [], None
    epoch_ms, val_hist = [], []
    cur = torch.cuda.current_stream()
    bufs = {}                                                    # a widened training batch lives in the same two tensors every iteration
    # --strong_augs / --weak_augs on --data_pt batches; None: bypassed, or (resident) run by the launch that forms the batch
    augment = None if task.resident else stage_for(args, with_mask=task.with_mask, rank=rank)
    resize = dataset_folder.stage_for(args, task.with_mask)      # --data_root: PIL's resize of the decoded files, one launch per batch; else None
    criterion, to_input, with_mask, ahead, in_channels = task.criterion, task.to_input, task.with_mask, task.data_parallel, args.in_channels
    lr_max, lr_min, clock = args.lr, args.lr_min, time.perf_counter
    batches = None
    if ahead:
        dm.set_epoch(0)
        batches = iter(train_pf)
    for epoch in range(args.epochs):
        torch.cuda.synchronize()
        t0, w0, enq, n_it = clock(), train_pf.wait_s, 0.0, 0
        if augment is not None:
            augment.set_epoch(epoch)
        if task.resident:
            train_pf.set_epoch(epoch)
        if not ahead:
            batches = iter(train_pf)
        for images, labels, ready in batches:
            t1 = clock()
            cur.wait_event(ready)
            if resize is not None:
                images, labels = resize(images, labels)
            if augment is not None:
                images, labels = augment(images, labels) if with_mask else (augment(images)[0], labels)
            images, labels = to_input(images, labels, in_channels, bufs)
            # scheduler.step() follows optimizer.step() in the reference: iteration i runs at the closed form's value for i
            loss, _ = segmentation_step(model, criterion, opt, images, labels, lr=cosine_lr(lr_max, lr_min, iter_num, max_iters), **kwargs_for(images.shape[0]))
            if iter_num % 10 == 0:                              # the reference's loss.item(), without the host read: flushed at validation time
                logged.append((iter_num, loss, cosine_lr(lr_max, lr_min, iter_num + 1, max_iters)))
            iter_num += 1
            n_it += 1
            enq += clock() - t1
        t2 = clock()
        torch.cuda.synchronize()
        epoch_ms.append({"ms": (clock() - t0) * 1e3, "updates": n_it})
        if task.loop_timings:
            epoch_ms[-1].update(loader_wait_ms=(train_pf.wait_s - w0) * 1e3, enqueue_ms=enq * 1e3, drain_ms=(clock() - t2) * 1e3)
        validate = (epoch > 0 and epoch % args.val_every == 0) or (epoch == args.epochs - 1)
        if ahead and epoch + 1 < args.epochs:                    # the next epoch's first batches load while this one validates
            dm.set_epoch(epoch + 1)
            batches = iter(train_pf)
        if not validate:
            continue

        model.eval()
        for it, l, lr in logged:
            writer.add_scalar(f"{args.exp}/train_loss", l, it)
            if task.lr_scalar:
                writer.add_scalar(f"{args.exp}/lr", lr, it)
        last = float(logged[-1][1]) if logged else last
        logged = []
        accumulator = task.metrics(criterion=criterion, num_classes=args.num_classes)
        roc_dir = os.path.join(args.train_snapshot_path, "roc_curves") if task.roc_csv and rank == 0 else None
        stats = _split_pass(task, model, val_pf, accumulator, args, kwargs_for, writer, "val", iter_num, roc_dir, resize)
        val_hist.append({"epoch": epoch, **stats})
        if stats[task.best] > best:
            patience, best = 0, stats[task.best]
            if rank == 0:
                torch.save(model.checkpoint_dict(), best_path)
        else:
            patience += 1
        if patience >= args.patience:
            logging.info(f"\nEarly stopping at epoch {epoch + 1}")
            if task.stop_twice:
                logging.info(f"Early stopping triggered at epoch {epoch + 1}")
            break
        logging.info(f"\titer: {iter_num}, loss: {stats['loss']:.4f}, " + task.line(stats))
        val_hist[-1]["test"] = _split_pass(task, model, test_pf, accumulator, args, kwargs_for, writer, "test", iter_num, resize=resize)
        model.train()

    writer.close()
    for pf in (train_pf, val_pf, test_pf):
        pf.close()                                               # an epoch prefetched and then abandoned by early stopping
    dm.shutdown()
    if world > 1:
        from uia_hip import ops
        import torch.distributed as dist
        dist.barrier()
        ops.comm_destroy()
    if rank == 0 and not os.path.exists(best_path):
        logging.warning(f"no validation improved on {task.best_words} of 0.0: saving the last iterate as best_model.pth (the reference has no checkpoint then "
                        "and fails in test())")
        torch.save(model.checkpoint_dict(), best_path)
    out = {"iters": iter_num, task.best_name: best, "last_loss": last, "epochs": epoch_ms, "augmented_images": augment.augmented if augment is not None else 0}
    if task.resident:
        out.update(augmented_images=train_pf.augmented, original_train_count=dm.original_train_count, sampled_train_count=dm.sampled_train_count)
    if task.data_parallel:
        out.update(rank=rank, world=world)
    if task.val_history:
        out["val"] = val_hist
    if args.stats_json and rank == 0:
        import json
        with open(args.stats_json, "w") as f:
            json.dump(out, f)
    return out


@torch.no_grad()
def test(args, task, prepare, forward_kwargs=None):
    logging.info("Start testing")
    rank = dist_env()[0] if task.data_parallel else 0
    dm = _data_module(args, task, 0, 1)                          # every rank evaluates the whole split
    testloader = dm.test_dataloader()
    dm.start_workers()
    _bind(args, task)
    model = prepare(args)
    saved_best = os.path.join(args.train_snapshot_path, "best_model.pth")
    model.load_checkpoint(torch.load(saved_best, map_location="cpu"))
    UF.WEIGHTS.bump()
    model.eval()
    kwargs_for = forward_kwargs(args) if forward_kwargs is not None else _no_kwargs
    viz = None
    if rank == 0:
        viz_path = fresh_viz_dir(args)
        if task.visualize and getattr(args, "viz", True):
            viz = SegVisualizer(viz_path, args.batch_size, args.img_size)
    accumulator = task.metrics(criterion=task.criterion, num_classes=args.num_classes)
    test_pf = _prefetcher(args, task, testloader)
    try:
        evaluate(task, model, test_pf, accumulator, args.in_channels, kwargs_for, viz, dm.test_dataset.name_of, dataset_folder.stage_for(args, task.with_mask))
        stats = accumulator.compute()
    finally:
        if viz is not None:
            viz.close()                                          # the last files are on disk before the folder moves; a writer's exception surfaces here
    accumulator.reset()
    test_pf.close()
    dm.shutdown()
    stats["results_csv"] = task.report(args, stats, saved_best, rank)
    return stats


def run(args, task, prepare, forward_kwargs=None):
    """main() of every entry point: seeds, the two run directories, train unless --test, then ALWAYS test.  Returns train()'s dict with test()'s under "test"."""
    if task.resident:
        dataset_folder.refuse(args, "a few-shot entry (its training set is resident on the device)")
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
        out = train(args, task, prepare, forward_kwargs)
    setup_logging(args, args.test_snapshot_path)
    out["test"] = test(args, task, prepare, forward_kwargs)
    return out
