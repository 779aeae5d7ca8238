"""BiomedCLIP image-text retrieval on ROCOv2 on the MI355X HIP path — counterpart of the reference's src/models/biomedclip/retrieval.py, the fifth
step of its BiomedCLIP pipeline (scripts/biomedclip.sh).

Kept from the reference: the command line (:20-110), the three ways a model is loaded (:113-176: `--ckpt` a fine-tuned state dict under "state_dict" /
"model_state_dict" / "model" or bare, loaded non-strictly; else `--lora_weights`; else `--mona_weights`, both by parameter NAME), fp32 features of the
whole split (:179-213), the metric keys, the result block, results.csv (`Metric,Value`, %.2f) and the `<time>_rsum=<rsum>` folder the log moves into
(:216-297).  The two modules the reference imports and never shipped are src/datasets/rocov2.py and src/utils/retrieval_metrics.py of this build.

Different: the features stay on the device (the reference moves every batch to the CPU, :205-206) and the metrics are two HIP calls that never form
the n x n score matrix (uia_retrieval_ranks / uia_retrieval_stats), one host copy for the lot.  Data: `--synthetic` or `--data_pt {"images", "captions"}`.

Added, off by default: `--topk K` lists each query's K best candidates in both directions (topk_i2t.csv, topk_t2i.csv beside results.csv, and "topk" in
features.pth) from the fused top-K kernel (uia_retrieval_topk: the same score tiles, equal scores by candidate index), and logs hit@K, the share of queries
whose own pair is in their list (at most R@K, whose tie rule is optimistic); `--queries_txt FILE` retrieves the K best images of the split for each line of
free text (topk_queries.csv).  Neither changes the metrics or results.csv.
"""
import argparse
import logging
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.adapters import inject_lora_to_biomedclip, inject_mona_variant_to_open_clip
from src.adapters.checkpoint import load_adapter_by_name
from src.datasets.rocov2 import ROCOv2DataModule
from src.third_party.biomedclip.model import SyntheticTokenizer, create_biomedclip
from src.utils.retrieval_metrics import compute_retrieval_metrics, hit_at_k, log_retrieval_metrics, retrieve_topk, write_topk_csv
from src.utils.tools import default_device, parse_config, setup_logging
from uia_hip import functional as UF

TOPK_MAX = 32                                           # the limit of uia_retrieval_topk


def get_args(argv=None):
    parser = argparse.ArgumentParser("BiomedCLIP Text-Image Retrieval on ROCOv2")
    # Model related
    parser.add_argument("--ckpt", type=str, default=None, help="Path to finetuned model checkpoint (if None, use pretrained BiomedCLIP)")
    parser.add_argument("--model_name", type=str, default="hf-hub:microsoft/BiomedCLIP-PubMedBERT_256-vit_base_patch16_224", help="Model name for open_clip")
    # MONA adapter related
    parser.add_argument("--mona_weights", type=str, default=None, help="Path to pretrained MONA weights (if provided, inject and load MONA adapters)")
    parser.add_argument("--mona_bottleneck", type=int, default=64, help="MONA bottleneck dimension")
    parser.add_argument("--mona_layers", type=int, default=None, help="Number of layers to inject MONA (None=all)")
    parser.add_argument("--mona_variant", type=str, default="freq_enhanced", choices=["baseline", "fractional", "noise_aware", "freq_enhanced", "hybrid"],
                        help="MONA variant type")
    # LoRA adapter related
    parser.add_argument("--lora_weights", type=str, default=None, help="Path to pretrained LoRA weights")
    parser.add_argument("--lora_r", type=int, default=16, help="LoRA rank")
    parser.add_argument("--lora_alpha", type=int, default=32, help="LoRA alpha")
    # Data related
    parser.add_argument("--img_size", type=int, default=224, help="Image size")
    parser.add_argument("--batch_size", type=int, default=128, help="Batch size for evaluation")
    parser.add_argument("--num_workers", type=int, default=8, help="Number of data loading workers")
    parser.add_argument("--split", type=str, default="test", choices=["train", "validation", "test"], help="Dataset split to evaluate on")
    parser.add_argument("--cache_dir", type=str, default="./data/rocov2_cache", help="Directory to cache ROCOv2 dataset")
    parser.add_argument("--max_samples", type=int, default=None, help="Maximum samples to evaluate (for debugging, None=all)")
    # Retrieval settings
    parser.add_argument("--k_values", type=int, nargs="+", default=[1, 2, 5, 10], help="K values for Recall@K metrics")
    # Experiment settings
    parser.add_argument("--exp", type=str, default="biomedclip_retrieval", help="Experiment name")
    parser.add_argument("--seed", type=int, default=42, help="Random seed")
    parser.add_argument("--device", type=str, default=default_device())
    # Output settings
    parser.add_argument("--save_features", action="store_true", help="Save extracted features to disk")
    parser.add_argument("--output_dir", type=str, default=None, help="Directory to save results (default: runs/{exp})")
    # additions of this build
    parser.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"], help="operand type of the towers' GEMMs; the features and the retrieval are fp32 either way")
    parser.add_argument("--synthetic", action="store_true")
    parser.add_argument("--synthetic_test", type=int, default=64, help="pairs per split of --synthetic")
    parser.add_argument("--data_pt", type=str, default=None, help=".pt with {'images': [N,1|3,S,S], 'captions': [N] str}")
    parser.add_argument("--data_root", type=str, default=None, help="refused here: the folder loader serves the supervised classification / segmentation entries")
    parser.add_argument("--ckpt_path", type=str, default=None, help="pretrained BiomedCLIP state dict (the reference downloads it by --model_name)")
    parser.add_argument("--model_config", type=str, default=None)
    parser.add_argument("--topk", type=int, default=0, help="list each query's K best candidates (topk_i2t.csv, topk_t2i.csv); 0 = off, at most 32")
    parser.add_argument("--queries_txt", type=str, default=None, help="one free-text query per line: the K best images of the split for each (topk_queries.csv); needs --topk")
    args = parser.parse_args(argv)
    if not 0 <= args.topk <= TOPK_MAX:
        parser.error(f"--topk {args.topk}: the listing holds at most {TOPK_MAX} candidates per query")
    if args.queries_txt is not None and args.topk == 0:
        parser.error("--queries_txt needs --topk K")
    return args


def load_model(args):
    """reference :113-176: the pretrained model, then ONE of fine-tuned weights / LoRA / Mona, in that order of precedence; fp32 parameters, eval mode."""
    cfg = parse_config(args.model_config) if args.model_config else None
    state = torch.load(args.ckpt_path, map_location="cpu") if args.ckpt_path else None
    model = create_biomedclip(state_dict=state, config=cfg, seed=args.seed)
    tokenizer = SyntheticTokenizer(256 if cfg is None else cfg["text_cfg"]["max_position_embeddings"])
    if args.ckpt is not None and os.path.exists(args.ckpt):
        logging.info(f"Loading finetuned weights from: {args.ckpt}")
        checkpoint = torch.load(args.ckpt, map_location="cpu")
        for key in ("state_dict", "model_state_dict", "model"):
            if key in checkpoint:
                checkpoint = checkpoint[key]
                break
        model.load_state_dict(checkpoint, strict=False)
        UF.WEIGHTS.bump()                               # operand copies of the replaced weights are stale
        logging.info("✓ Finetuned weights loaded")
    elif args.lora_weights is not None and os.path.exists(args.lora_weights):
        logging.info(f"Injecting LoRA adapters (r={args.lora_r}, alpha={args.lora_alpha})")
        inject_lora_to_biomedclip(model, lora_r=args.lora_r, lora_alpha=args.lora_alpha, lora_dropout=0.0)
        n = load_adapter_by_name(model, args.lora_weights, "lora_state_dict")
        logging.info(f"✓ Loaded {n} LoRA parameters from {args.lora_weights}")
    elif args.mona_weights is not None and os.path.exists(args.mona_weights):
        logging.info(f"Injecting MONA adapters (variant: {args.mona_variant})")
        inject_mona_variant_to_open_clip(model, variant=args.mona_variant, bottleneck_dim=args.mona_bottleneck, num_layers=args.mona_layers)
        n = load_adapter_by_name(model, args.mona_weights, "mona_state_dict")
        logging.info(f"✓ Loaded {n} MONA parameters from {args.mona_weights}")
    for p in model.parameters():
        p.requires_grad = False
    model.float()
    model.to(args.device)
    model.eval()
    return model, tokenizer


@torch.no_grad()
def extract_features(model, tokenizer, dataloader, args):
    """(image_features [N, D], text_features [N, D], captions list of N): fp32, on args.device."""
    all_image_features, all_text_features, all_captions = [], [], []
    for images, captions, _ in dataloader:
        images = images.to(args.device)
        texts = tokenizer(captions).to(args.device)
        all_image_features.append(model.encode_image(images).float())
        all_text_features.append(model.encode_text(texts).float())
        all_captions.extend(captions)
    return torch.cat(all_image_features, dim=0), torch.cat(all_text_features, dim=0), all_captions


def result_rows(k_values, metrics):
    """The rows of results.csv in the reference's order (:229-248)."""
    rows = []
    for d, tag in (("i2t", "I2T"), ("t2i", "T2I")):
        rows += [(f"{tag}_R@{k}", metrics[f"{d}_r@{k}"]) for k in k_values]
        rows += [(f"{tag}_MedR", metrics[f"{d}_medr"]), (f"{tag}_MeanR", metrics[f"{d}_meanr"])]
    rows.append(("rSum", metrics["rsum"]))
    return rows


@torch.no_grad()
def topk_listings(model, tokenizer, image_features, text_features, args):
    """--topk: {"i2t": (idx, score), "t2i": (idx, score)} and, with --queries_txt, "queries" (the file's lines against the images) with the lines
    themselves; CPU tensors [n, K], K = min(--topk, n).  One line per paired direction with hit@K for each --k_values entry <= K."""
    n = image_features.shape[0]
    K = min(args.topk, n)
    listings = {}
    for d, title, q, g in (("i2t", "Image-to-Text", image_features, text_features), ("t2i", "Text-to-Image", text_features, image_features)):
        idx, score = retrieve_topk(q, g, K, normalize=True)
        hits = hit_at_k(idx, args.k_values)
        logging.info(f"[{args.split}] {title} top-{K} listing: " + "  ".join(f"hit@{k}: {v:.2f}" for k, v in hits.items()))
        listings[d] = (idx.cpu(), score.cpu())
    lines = None
    if args.queries_txt is not None:
        with open(args.queries_txt) as f:
            lines = [ln.strip() for ln in f if ln.strip()]
        if not lines:
            raise RuntimeError(f"--queries_txt {args.queries_txt}: no query lines")
        feats = [model.encode_text(tokenizer(lines[i:i + args.batch_size]).to(args.device)).float() for i in range(0, len(lines), args.batch_size)]
        idx, score = retrieve_topk(torch.cat(feats, dim=0), image_features, K, normalize=True)
        listings["queries"] = (idx.cpu(), score.cpu())
    return listings, lines


def save_results(args, metrics, image_features=None, text_features=None, captions=None, listings=None, query_lines=None):
    """reference :216-297: <output_dir>/<time>_rsum=<rsum>/ with results.csv, the log and, with --save_features, features.pth; with --topk the listings
    topk_i2t.csv / topk_t2i.csv (/ topk_queries.csv); returns the folder."""
    import datetime
    import shutil
    backup_folder = os.path.join(args.output_dir, f"{datetime.datetime.now().strftime('%Y_%m_%d_%H_%M_%S')}_rsum={metrics['rsum']:.2f}")
    base, n = backup_folder, 1
    while os.path.exists(backup_folder):                # two runs within one second with the same rsum
        n += 1
        backup_folder = f"{base}__{n}"
    os.makedirs(backup_folder)
    csv_path = os.path.join(backup_folder, "results.csv")
    with open(csv_path, "w") as f:
        f.write("Metric,Value\n" + "".join(f"{name},{value:.2f}\n" for name, value in result_rows(args.k_values, metrics)))
    logging.info(f"Results saved to: {csv_path}")
    result_str = f"\n{'=' * 50}\n"
    for d, title in (("i2t", "Image-to-Text"), ("t2i", "Text-to-Image")):
        result_str += f"{title} Retrieval:\n"
        for k in args.k_values:
            result_str += f"  R@{k}: {metrics[f'{d}_r@{k}']:.2f}%\n"
        result_str += f"  MedR: {metrics[f'{d}_medr']:.1f}\n"
        result_str += f"  MeanR: {metrics[f'{d}_meanr']:.1f}\n\n"
    result_str += f"rSum: {metrics['rsum']:.2f}\n"
    result_str += f"{'=' * 50}\n"
    logging.info(result_str)
    if listings:
        for d, (idx, score) in listings.items():
            listing_path = os.path.join(backup_folder, f"topk_{d}.csv")
            write_topk_csv(listing_path, idx, score, query_lines if d == "queries" else captions, d)
            logging.info(f"Top-{idx.shape[1]} listing saved to: {listing_path}")
    if args.save_features and image_features is not None and text_features is not None:
        features_file = os.path.join(backup_folder, "features.pth")
        saved = {"image_features": image_features.cpu(), "text_features": text_features.cpu(), "captions": captions, "metrics": metrics}
        if listings:
            saved["topk"] = {d: listings[d] for d in ("i2t", "t2i")}
        torch.save(saved, features_file)
        logging.info(f"Features saved to: {features_file}")
    for h in list(logging.getLogger().handlers):
        h.flush()
    log_path = os.path.join(args.output_dir, "log.log")
    if os.path.exists(log_path):
        shutil.move(log_path, os.path.join(backup_folder, "log.log"))
    return backup_folder


def main(argv=None):
    args = get_args(argv)
    from src.datasets import folder
    folder.refuse(args, "retrieval")
    if args.output_dir is None:
        args.output_dir = f"runs/{args.exp}/test"
    os.makedirs(args.output_dir, exist_ok=True)
    setup_logging(args, args.output_dir)
    torch.manual_seed(args.seed)
    UF.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    model, tokenizer = load_model(args)
    data_module = ROCOv2DataModule(args, cache_dir=args.cache_dir, max_samples=args.max_samples, seed=args.seed)
    if args.split == "train":
        dataloader = data_module.train_dataloader(shuffle=False)
    elif args.split == "validation":
        dataloader = data_module.val_dataloader()
    else:
        dataloader = data_module.test_dataloader()
    image_features, text_features, captions = extract_features(model, tokenizer, dataloader, args)
    metrics = compute_retrieval_metrics(image_features, text_features, k_values=args.k_values, normalize=True)
    log_retrieval_metrics(metrics, prefix=args.split)
    listings, query_lines = topk_listings(model, tokenizer, image_features, text_features, args) if args.topk > 0 else (None, None)
    args.backup_folder = save_results(args, metrics, image_features, text_features, captions, listings, query_lines)
    logging.info("✓ Retrieval evaluation complete")
    return metrics


if __name__ == "__main__":
    main()
