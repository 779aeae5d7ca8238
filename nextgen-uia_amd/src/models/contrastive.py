"""The contrastive fine-tune loop of the four CLIP-family entry points (src/models/{biomedclip,metaclip,clip,unimedclip}/finetune.py): `train`, `run` (the body
of every `main`), the build's shared flags (`add_build_args`), the opt-in post-training zero-shot evaluation (`add_zero_shot_flags`, `run_zero_shot_evaluation`)
and the two recipes the loop reads (`BIOMEDCLIP`, `CLIP_FAMILY`).

What the reference repeats per family (src/models/biomedclip/finetune.py:211-361; src/models/metaclip/finetune.py:92-218, which its clip/ and unimedclip/ entries
repeat verbatim): per loader batch InfoNCE, non-finite batches skipped, clip_grad_norm_ -> AdamW -> cosine LR at every accumulation boundary, a validation pass per
epoch in eval mode, the best-val checkpoint (strict <), early stopping by --patience, runs/<exp>/{log.log,best_model.pth}.  On the measured step: every loader batch
goes through engine.ContrastiveLoop.micro (contrastive_micro: text tower on its own stream, image tower in two slices, three-byte residual gradients; guarded
accumulate) and every accumulation boundary through the device-guarded clip + AdamW, the same functions bench.py times.  The host reads nothing per batch: the
non-finite skip is decided on the device, the epoch's loss sum / counts / skipped indices come back in ONE read at the end of the epoch, validation reads once per
pass, batches arrive through a double-buffered prefetcher.  Data parallel under torch.distributed.run: one process per GPU, rank 0 saves.

Data: --data_pt, then --synthetic (src/datasets/finetune.py), then --finetune_root, the reference's caption folders as released (src/datasets/captions.py: workers
decode into a ring of byte slots, `RgbResizeStage` behind the prefetcher's event makes the [B, 3, S, S] batch in one uia_resize_batch_rgb launch); --data_root is
refused.  --tokenizer_json puts a tokenizer file's ids in the stand-in tokenizer's place (src/utils/tokenizer_file.py, through each family's `make_tokenizer`).

What differs by family and cannot be read from `args` is a field of `Recipe`; what can is read from `args` (--accumulation_steps, default 1; --grad_clip, default 1.0;
--method, default "mona": what the checkpoint holds).  What differs by model is an argument: `prepare_model(args) -> (model, tokenizer)` and `make_tokenizer(args)`.
"""
import json
import logging
import math
import os
import random
import subprocess
import sys
import time
from dataclasses import dataclass

import numpy as np
import torch

from src.datasets import captions
from src.datasets import finetune as dataset_finetune
from src.losses import InfoNCELoss
from src.utils.tools import model_summary, setup_logging
from uia_hip import functional as UF
from uia_hip.engine import ContrastiveLoop, DevicePrefetcher, FlatAdapterOptimizer, bind_device, dist_env, init_data_parallel, sum_over_ranks

ZERO_SHOT_DATASETS = ("LN-INT", "LN-EXT", "BUSI")               # reference metaclip/finetune.py:256


@dataclass(frozen=True)
class Recipe:
    figures: object                 # (train sum, finite train batches, train batches, val sum, finite val batches, val batches, world) -> the epoch's (train, val) figures, equal on every rank
    skip_line: str                  # the warning per skipped batch ...
    epoch_line: str                 # ... the line per epoch ...
    saved_line: str
    stop_line: str
    done_line: str                  # ... and the last line; all formatted with the names train() gives them
    updates_name: str               # the key of the update count in train()'s dict
    start_line: str = None          # logged once before the first epoch
    features: object = None         # (image features, text features) -> what the loss takes, in training and in validation; None: as encoded
    discard_on_skip: bool = False   # a skipped batch also discards what its cycle had accumulated (the reference zeroes the gradients before every backward)
    log_first: bool = False         # the epoch line comes before the best / patience decision and shows the previous best
    ranks_in_result: bool = False   # "rank" / "world" in train()'s dict
    zero_shot_script: object = None  # --zero_shot_eval: the family's zero_shot.py ...
    zero_shot_flags: object = None   # ... and args -> its model flags


def _ratio_of_sums(train_sum, train_ok, train_n, val_sum, val_ok, val_n, world):
    """Sums over ranks, then finite losses over the count of finite ones (0.0 if none)."""
    val_sum, val_ok, train_sum, train_ok = sum_over_ranks(val_sum, val_ok, train_sum, train_ok)
    return (train_sum / train_ok if train_ok else 0.0), (val_sum / val_ok if val_ok else 0.0)


def _mean_per_batch(train_sum, train_ok, train_n, val_sum, val_ok, val_n, world):
    """Finite losses over the loader's length (a skipped batch stays in the denominator), then the mean over ranks."""
    val, train = (v / world for v in sum_over_ranks(val_sum / max(1, val_n), train_sum / max(1, train_n)))
    return train, val


def _normalise(fi, ft):
    """reference metaclip/finetune.py:147-148: the entry point L2-normalises both feature matrices before the loss"""
    return fi / fi.norm(dim=-1, keepdim=True), ft / ft.norm(dim=-1, keepdim=True)


BIOMEDCLIP = Recipe(figures=_ratio_of_sums, ranks_in_result=True, updates_name="updates",
                    start_line="Gradient accumulation steps: {accumulation_steps}; updates per epoch: {updates_per_epoch}; world: {world}",
                    skip_line="Non-finite loss detected at batch {batch} in epoch {epoch}, skipping batch",
                    epoch_line="Epoch {epoch}: Train={train:.4f}, Val={val:.4f}, Best={best:.4f}",
                    saved_line="\nBest model saved at epoch {epoch} with validation loss {best:.4f}",
                    stop_line="\nEarly stopping at epoch {epoch} as validation loss did not improve for {patience} epochs.",
                    done_line="\n✓ Training completed! Best validation loss: {best:.4f} at epoch {best_epoch}")
# MetaCLIP, OpenAI CLIP, UniMed-CLIP: no accumulation or clip flag (one batch per update, norm 1.0); an entry adds its zero_shot.py
CLIP_FAMILY = Recipe(figures=_mean_per_batch, features=_normalise, discard_on_skip=True, log_first=True, updates_name="iters",
                     skip_line="Non-finite loss detected at iteration {updates}, skipping batch",          # the count from before the epoch's updates
                     epoch_line="Epoch {epoch}/{epochs}: Train={train:.4f}, Val={val:.4f}, Best={best:.4f}",
                     saved_line="Best model saved at epoch {epoch}", stop_line="Early stopping triggered at epoch {epoch}",
                     done_line="\n✓ Training completed! Best loss: {best:.4f} (epoch {best_epoch})")


def add_build_args(p):
    """The additions of this build shared by the four entries (beside the reference's flags)."""
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"], help="operand precision of the HIP kernels")
    p.add_argument("--synthetic", action="store_true", help="synthetic image-caption pairs (no dataset files needed)")
    p.add_argument("--synthetic_train", type=int, default=512)
    p.add_argument("--synthetic_val", type=int, default=128)
    p.add_argument("--data_pt", type=str, default=None, help=".pt with {'images': [N,3,S,S], 'texts': [str]}")
    p.add_argument("--data_root", type=str, default=None, help="refused here: the folder loader serves the supervised classification / segmentation entries")
    p.add_argument("--finetune_root", type=str, default=None, help="the reference's caption folders as released: DIR/{medpix_dataset,pmc_curd_dataset}/{<name>.csv,images/} "
                   "(taken after --data_pt and --synthetic)")
    p.add_argument("--tokenizer_json", type=str, default=None, help="a tokenizer file of the `tokenizers` library: real token ids in place of the stand-in tokenizer")
    p.add_argument("--model_config", type=str, default=None, help="python literal overriding the model geometry, in the form the family's model constructor takes (tests)")


def add_zero_shot_flags(p):
    p.add_argument("--zero_shot_eval", action="store_true", help="after training, evaluate best_model.pth zero-shot on LN-INT, LN-EXT and BUSI")
    p.add_argument("--zero_shot_data_pt", type=str, default=None, help=".pt with {'images', 'labels'}: the evaluation's --data_pt (--synthetic is passed on as it is)")
    p.add_argument("--zero_shot_timeout", type=int, default=3600, help="seconds one evaluation may take")


def _save_checkpoint(model, args, save_path):
    method = getattr(args, "method", "mona")
    if method == "full":                                         # reference biomedclip/finetune.py:200-208: the whole state dict
        torch.save(model.state_dict(), save_path)
    else:                                                        # the adapter's parameters by name ("mona" / "lora"): the checkpoint wire format
        torch.save({n: p.data.clone() for n, p in model.named_parameters() if method in n.lower()}, save_path)


def train(args, recipe, prepare_model, make_tokenizer):
    rank, _, world = dist_env()
    if not torch.cuda.is_initialized():                         # a fresh CLI process (not a caller that is already running other GPU / CPU work in this process)
        torch.set_num_threads(max(1, min(4, torch.get_num_threads())))      # host tensor work here is one staging copy per batch; the default (every logical CPU of the node) oversubscribes a job's CPU share
    folders = captions.chosen(args)                             # --finetune_root: workers decode, the batch is made on the device (src/datasets/captions.py)
    if folders and not getattr(args, "tokenizer_json", None):
        logging.warning("--finetune_root without --tokenizer_json: the captions go through the stand-in tokenizer, whose ids mean nothing to a pretrained text tower")
    dm = (captions if folders else dataset_finetune).DataModule(args, rank=rank, world=world, tokenizer=make_tokenizer(args))
    trainloader, valloader = dm.train_dataloader(), dm.val_dataloader()
    dm.start_workers()                                         # loader worker processes are forked BEFORE this process touches the GPU
    bind_device(args)                                          # data parallel: cuda:LOCAL_RANK before anything is allocated
    UF.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    UF.set_dropout_seed(args.seed + 7919 * rank)                # ranks draw different dropout masks, like different micro-batches
    model, tokenizer = prepare_model(args)
    model.train()
    logging.info(model_summary({"model": model}))
    criterion = InfoNCELoss(temperature=args.temperature)
    accumulation_steps = getattr(args, "accumulation_steps", 1)
    opt = FlatAdapterOptimizer([(n, p) for n, p in model.named_parameters() if p.requires_grad], lr=args.lr,
                               betas=(args.beta1_adam, args.beta2_adam), weight_decay=args.weight_decay, max_norm=getattr(args, "grad_clip", 1.0))
    if world > 1:
        init_data_parallel(opt)
    updates_per_epoch = math.ceil(len(trainloader) / accumulation_steps)
    if recipe.start_line:
        logging.info(recipe.start_line.format(accumulation_steps=accumulation_steps, updates_per_epoch=updates_per_epoch, world=world))
    loop = ContrastiveLoop(model, criterion, opt, accumulation_steps=accumulation_steps, lr=args.lr, lr_min=args.lr_min, total_updates=updates_per_epoch * args.epochs,
                           features=recipe.features, discard_on_skip=recipe.discard_on_skip)
    features = recipe.features or (lambda fi, ft: (fi, ft))
    if folders:
        train_pf, val_pf = captions.CaptionPrefetcher(trainloader, args.device), captions.CaptionPrefetcher(valloader, args.device)
        stage = captions.RgbResizeStage(args.img_size)
    else:
        train_pf, val_pf, stage = DevicePrefetcher(trainloader, tokenizer, args.device), DevicePrefetcher(valloader, tokenizer, args.device), None

    best_loss, best_epoch, patience = float("inf"), 0, 0
    avg_train, update_count, epoch_ms = 0.0, 0, []
    dm.set_epoch(0)
    batches = iter(train_pf)                                    # the producer starts now: the first batches are resident when the epoch begins
    for epoch in range(args.epochs):
        model.train()
        loop.begin_epoch(len(trainloader))
        torch.cuda.synchronize()
        t0, w0, enq, gw0 = time.perf_counter(), train_pf.wait_s, 0.0, getattr(opt, "gpu_wait_s", 0.0) + UF._STATE.get("gpu_wait_s", 0.0)
        for batch_idx, (images, tokens, ready) in enumerate(batches):
            t1 = time.perf_counter()
            if stage is not None:                                # the ragged batch -> [B, 3, S, S]: one launch behind the prefetcher's event
                torch.cuda.current_stream().wait_event(ready)
                images = stage(images)
            loop.micro(images, tokens, batch_idx, ready=ready)
            enq += time.perf_counter() - t1
        t2 = time.perf_counter()
        g = loop.end_epoch()                                     # the epoch's one host read (reference: loss.item() per batch)
        epoch_ms.append({"ms": (time.perf_counter() - t0) * 1e3, "updates": g["updates"] - update_count, "batches": len(trainloader),
                         "loader_wait_ms": (train_pf.wait_s - w0) * 1e3, "enqueue_ms": enq * 1e3, "drain_ms": (time.perf_counter() - t2) * 1e3,
                         "host_waited_for_gpu_ms": (getattr(opt, "gpu_wait_s", 0.0) + UF._STATE.get("gpu_wait_s", 0.0) - gw0) * 1e3})
        for i in g["skipped_batches"]:
            logging.warning(recipe.skip_line.format(batch=i, epoch=epoch + 1, updates=update_count))
        update_count = g["updates"]
        if epoch + 1 < args.epochs:                              # next epoch's first batches load while this epoch validates
            dm.set_epoch(epoch + 1)
            batches = iter(train_pf)
        model.eval()
        vstat = torch.zeros(2, device=args.device)               # the sum of the finite losses, their count
        with torch.no_grad():
            for images, tokens, ready in val_pf:
                torch.cuda.current_stream().wait_event(ready)
                if stage is not None:
                    images = stage(images)
                loss = criterion(*features(model.encode_image(images), model.encode_text(tokens)))
                ok = torch.isfinite(loss)
                vstat += torch.stack([torch.where(ok, loss, torch.zeros_like(loss)), ok.to(loss.dtype)])
        val_sum, val_ok = vstat.tolist()
        # every rank evaluated its own shard: the figures are reduced over the ranks, so that the checkpoint / patience / early-stop decisions below are
        # identical on every rank (a rank that stopped alone would strand the others)
        avg_train, avg_val = recipe.figures(g["loss_sum"], g["epoch_accumulated"], len(trainloader), val_sum, val_ok, len(valloader), world)
        if recipe.log_first:
            logging.info(recipe.epoch_line.format(epoch=epoch + 1, epochs=args.epochs, train=avg_train, val=avg_val, best=best_loss))
        if avg_val < best_loss:
            best_loss, patience, best_epoch = avg_val, 0, epoch
            if rank == 0:
                _save_checkpoint(model, args, os.path.join(args.train_snapshot_path, "best_model.pth"))
            logging.info(recipe.saved_line.format(epoch=epoch + 1, best=best_loss))
        else:
            patience += 1
        if not recipe.log_first:
            logging.info(recipe.epoch_line.format(epoch=epoch + 1, epochs=args.epochs, train=avg_train, val=avg_val, best=best_loss))
        if patience >= args.patience:
            logging.info(recipe.stop_line.format(epoch=epoch + 1, patience=args.patience))
            break
    logging.info(recipe.done_line.format(best=best_loss, best_epoch=best_epoch + 1))
    train_pf.close()                                           # an epoch prefetched ahead and abandoned by early stopping
    val_pf.close()
    dm.shutdown()
    if world > 1:
        from uia_hip import ops
        import torch.distributed as dist
        dist.barrier()
        ops.comm_destroy()
    out = {"best_val": best_loss, recipe.updates_name: update_count, "last_train": avg_train}
    if recipe.ranks_in_result:
        out.update(rank=rank, world=world)
    out["epochs"] = epoch_ms
    return out


def run_zero_shot_evaluation(args, script, extra=()):
    """reference metaclip/finetune.py:240-296, after train() has returned (loaders closed, communicator destroyed), on rank 0: `script` (the family's zero_shot.py) once
    per dataset on best_model.pth, each a fresh child process with the reference's arguments (:264-283) plus the adapter variant and this build's data and dtype
    flags; `extra`: the family's model flags.  A failed or timed-out child is logged and ends the loop.  -> the datasets evaluated."""
    if dist_env()[0] != 0:
        return []
    logging.info("=" * 50)
    logging.info("Starting Zero-shot Evaluation on Fine-tuned Model")
    logging.info("=" * 50)
    best = os.path.join(args.train_snapshot_path, "best_model.pth")
    if not os.path.exists(best):
        logging.error(f"Best model checkpoint not found at {best}")
        return []
    done = []
    for dataset in ZERO_SHOT_DATASETS:
        logging.info(f"\nEvaluating on {dataset} dataset...")
        cmd = [sys.executable, str(script), "--exp", f"{args.exp}", "--dataset", dataset, "--img_size", str(args.img_size), "--mona_weights", best,
               "--mona_bottleneck", str(args.mona_bottleneck), "--batch_size", "64", "--seed", str(args.seed), "--device", args.device,
               "--mona_variant", args.mona_variant, "--dtype", args.dtype, *extra]
        if args.synthetic:
            cmd.append("--synthetic")
        if args.zero_shot_data_pt:
            cmd += ["--data_pt", args.zero_shot_data_pt]
        if args.model_config:
            cmd += ["--model_config", args.model_config]
        logging.info(f"Running command: {' '.join(cmd)}")
        try:
            result = subprocess.run(cmd, capture_output=True, text=True, timeout=args.zero_shot_timeout)
        except subprocess.TimeoutExpired:
            logging.error(f"Zero-shot evaluation timed out for {dataset} after {args.zero_shot_timeout} s; the remaining datasets are not started")
            break
        logging.info(result.stdout)
        if result.returncode != 0:
            logging.error(f"Zero-shot evaluation failed for {dataset} (exit status {result.returncode}); the remaining datasets are not started")
            logging.error(f"Error: {result.stderr}")
            break
        if result.stderr:
            logging.warning(result.stderr)
        done.append(dataset)
    logging.info("Zero-shot Evaluation Completed")
    return done


def run(args, recipe, prepare_model, make_tokenizer):
    """main() of every entry point: seeds, runs/<exp>, train; then --zero_shot_eval and --stats_json (rank 0) where the entry has the flag.  Returns train()'s dict."""
    from src.datasets import folder
    folder.refuse(args, "the contrastive fine-tune")
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    args.train_snapshot_path = f"runs/{args.exp}"
    os.makedirs(args.train_snapshot_path, exist_ok=True)
    setup_logging(args, args.train_snapshot_path)
    out = train(args, recipe, prepare_model, make_tokenizer)
    if getattr(args, "zero_shot_eval", False):
        out["zero_shot"] = run_zero_shot_evaluation(args, recipe.zero_shot_script, recipe.zero_shot_flags(args))
    if getattr(args, "stats_json", None) and dist_env()[0] == 0:
        with open(args.stats_json, "w") as f:
            json.dump(out, f)
    return out
