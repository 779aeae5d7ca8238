"""Zero-shot classification: the loop that the four zero_shot.py entry points share (reference src/models/{biomedclip,metaclip,clip,unimedclip}/zero_shot.py,
one loop repeated four times: metaclip/zero_shot.py:116-264).

  * class text features once: every prompt of every class through the text tower, RAW, as one [T, E] matrix with the classes' row ranges;
  * every batch through the image tower and `uia_zero_shot_score` (csrc/zero_shot.hip: both normalisations, 100 · cosine, the per-class mean, in one launch)
    into ONE split-wide logits buffer on the device — nothing is read back per batch, and a row's logits do not depend on the batch it came in, so any
    --batch_size gives the same report;
  * ClassificationMetrics with torch.nn.CrossEntropyLoss (the reference's MetricAccumulator(type="cls")): acc / rec / pre / f1 / auc / loss, one host read;
    the exact ROC curve from `uia_binary_roc_curve`;
  * the reference's two diagnostics: a warning when the class prototypes are similar (> 0.95), and the collapse check on the normalised features of the
    first ten batches (top eigenvalue share of their second-moment matrix > 0.95).  The features are the kernel's `img_n` output, so there is no second pass
    over the data; they are copied to the host and torch.linalg.eigvalsh runs on the CPU — diagnostic only, as in the reference;
  * the "<Family> Zero-shot Results" table, and runs/<exp>/<dataset>/test/<time>_acc=<acc>/ with results.csv (Metric,Mean, %.2f), roc_curve.csv
    (fpr,tpr,threshold), roc_curve_<family>_zero_shot.png when matplotlib imports (skipped silently otherwise) and the log.

Data: --synthetic or --data_pt {"images", "labels"}; the reference's CSV / PIL loaders are outside this build."""
import json
import logging
import os

import torch

from src.models.zero_shot_prompt import ensemble_for
from src.utils.cls_metrics import ClassificationMetrics
from src.utils.tools import backup_test_run
from uia_hip import functional as UF
from uia_hip import ops

LESION_TYPES = ("benign", "malignant")
TITLES = {"biomedclip": "BiomedCLIP", "metaclip": "MetaCLIP", "clip": "CLIP", "unimedclip": "UniMedCLIP"}
DIAG_BATCHES = 10                                       # reference :202


def add_build_flags(p):
    """The flags this build adds to every zero-shot entry point (the BiomedCLIP entry's)."""
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--synthetic_test", type=int, default=64)
    p.add_argument("--data_pt", type=str, default=None, help=".pt with {'images': [N,3,S,S], 'labels': [N]}")
    p.add_argument("--data_root", type=str, default=None, help="refused here: the folder loader serves the supervised classification / segmentation entries")
    p.add_argument("--prompts_json", type=str, default=None, help='{"benign": [...], "malignant": [...]}')
    p.add_argument("--ckpt_path", type=str, default=None)
    p.add_argument("--model_config", type=str, default=None)


def load_test_split(args):
    """(images float [N,3,S,S], labels int64 [N]) on the host."""
    from src.datasets import folder
    folder.refuse(args, "zero-shot classification")
    if args.data_pt:
        blob = torch.load(args.data_pt)
        images, labels = blob["images"], blob["labels"].long()
        images = images.float() / 255.0 if images.dtype == torch.uint8 else images.float()
    elif args.synthetic:
        g = torch.Generator().manual_seed(args.seed)
        images = torch.rand(args.synthetic_test, 1, args.img_size, args.img_size, generator=g).repeat(1, 3, 1, 1)
        labels = torch.randint(0, 2, (args.synthetic_test,), generator=g)
    else:
        raise RuntimeError("no dataset: pass --synthetic or --data_pt")
    return images, labels


def prompts_of(args):
    return json.load(open(args.prompts_json)) if args.prompts_json else ensemble_for(args.dataset)


@torch.no_grad()
def class_prompt_features(model, tokenizer, prompts, device, classes=LESION_TYPES):
    """Raw text features of every prompt, class after class: ([T, E] fp32, class_off [C + 1])."""
    feats, off = [], [0]
    for c in classes:
        feats.append(model.encode_text(tokenizer(prompts[c]).to(device)).float())
        off.append(off[-1] + feats[-1].shape[0])
    return torch.cat(feats), off


def prototype_similarity(prm, off):
    """reference :151-153: <mean of class 0's normalised prompt features, mean of class 1's>; one host read, once per run."""
    t = prm / prm.norm(dim=-1, keepdim=True)
    return float(t[off[0]:off[1]].mean(0) @ t[off[1]:off[2]].mean(0))


def collapse_ratio(feats):
    """reference :219-226: the top eigenvalue's share of the spectrum of XᵀX / n over the sampled normalised features (host, diagnostic); None for <= 10 rows."""
    if len(feats) <= 10:
        return None
    x = feats.double()
    ev = torch.linalg.eigvalsh(x.T @ x / len(x)).abs()
    return float(ev.max() / ev.sum())


@torch.no_grad()
def evaluate(args, model, tokenizer):
    """-> (stats, logits [N, 2] on the device, (fpr, tpr, thresholds) on the host as float lists)."""
    images, labels = load_test_split(args)
    N = len(labels)
    prm, off = class_prompt_features(model, tokenizer, prompts_of(args), args.device)
    proto_sim = prototype_similarity(prm, off)
    if proto_sim > 0.95:
        logging.warning(f"Text prompts very similar: {proto_sim:.4f}")
    logits = torch.empty(N, len(off) - 1, device=args.device, dtype=torch.float32)
    sampled = []
    for b, r0 in enumerate(range(0, N, args.batch_size)):
        feats = model.encode_image(images[r0:r0 + args.batch_size].to(args.device))
        _, _, img_n = ops.zero_shot_score(feats, prm, off, out=logits, row=r0, want_probs=False, want_normalized=b < DIAG_BATCHES)
        if img_n is not None:
            sampled.append(img_n)
    metrics = ClassificationMetrics(criterion=torch.nn.CrossEntropyLoss(), num_classes=args.num_classes)
    metrics.update(logits, labels.to(args.device))
    stats = metrics.compute()
    stats["n"] = N
    fpr, tpr, thr = metrics.roc()
    ratio = collapse_ratio(torch.cat(sampled).cpu())
    if ratio is not None and ratio > 0.95:
        logging.warning(f"Features may be collapsed (ratio={ratio:.4f})")
    return stats, logits, (fpr.cpu().tolist(), tpr.cpu().tolist(), thr.cpu().tolist())


def save_roc_figure(path, fpr, tpr, title):
    """reference :236-243.  False when matplotlib is not installed: the figure is then left out."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    fig = plt.figure(figsize=(4, 4), dpi=600)
    plt.plot(fpr, tpr, linewidth=2)
    plt.plot([0, 1], [0, 1], "k--", linewidth=1)
    plt.xlabel("False Positive Rate", fontsize=12)
    plt.ylabel("True Positive Rate", fontsize=12)
    plt.grid(True, alpha=0.3)
    plt.title(title, fontsize=14)
    plt.tight_layout()
    fig.savefig(path, bbox_inches="tight")
    plt.close(fig)
    return True


def report(args, family, stats, roc):
    """The results table to the log, then the <time>_acc=<acc> folder; returns the folder."""
    rows = [("Acc", stats["acc"] * 100), ("Rec", stats["rec"] * 100), ("Pre", stats["pre"] * 100), ("F1", stats["f1"] * 100), ("AUC", stats["auc"] * 100)]
    bar = "=" * 50
    table = f"{'Metric':>6} {'Mean':>6}\n" + "".join(f"{m:>6} {a:6.2f}\n" for m, a in rows)
    logging.info(f"{bar}\n{TITLES[family]} Zero-shot Results\n{bar}\n{table}{bar}\n")
    csv_path = backup_test_run(args, f"acc={stats['acc'] * 100:.2f}", ["Metric,Mean"] + [f"{m},{a:.2f}" for m, a in rows], None)
    folder = os.path.dirname(csv_path)
    fpr, tpr, thr = roc
    with open(os.path.join(folder, "roc_curve.csv"), "w") as f:
        f.write("fpr,tpr,threshold\n" + "".join(f"{a!r},{b!r},{c!r}\n" for a, b, c in zip(fpr, tpr, thr)))
    save_roc_figure(os.path.join(folder, f"roc_curve_{family}_zero_shot.png"), fpr, tpr, f"{TITLES[family]} Zero-shot\nAUC = {stats['auc']:.4f}")
    return folder


def run(args, family, prepare_model):
    """test() of an entry point: dtype, model, evaluation.  -> (stats, logits on the device, roc)."""
    logging.info("=" * 50)
    logging.info(f"{TITLES[family]} Zero-shot Classification")
    logging.info("=" * 50)
    UF.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    model, tokenizer = prepare_model(args)
    stats, logits, roc = evaluate(args, model, tokenizer)
    logging.info(f"zero-shot {args.dataset}: acc {stats['acc'] * 100:.2f}  auc {stats['auc']:.4f}  loss {stats['loss']:.4f}  (n={stats['n']})")
    return stats, logits, roc


def main(args, family, prepare_model):
    """main() of an entry point: seeds, runs/<exp>/<dataset>/test, the evaluation, results.json and the report folder.  -> stats, with the folder as "report_dir"."""
    import random

    import numpy as np
    from src.utils.tools import setup_logging
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    args.test_snapshot_path = f"runs/{args.exp}/{args.dataset}/test"
    os.makedirs(args.test_snapshot_path, exist_ok=True)
    setup_logging(args, args.test_snapshot_path)
    stats, logits, roc = run(args, family, prepare_model)
    with open(os.path.join(args.test_snapshot_path, "results.json"), "w") as f:
        json.dump(stats, f)
    stats["report_dir"] = report(args, family, stats, roc)
    return stats
