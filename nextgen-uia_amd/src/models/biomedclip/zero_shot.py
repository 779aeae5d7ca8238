"""BiomedCLIP zero-shot classification on the MI355X HIP path — counterpart of
/root/reference/src/models/biomedclip/zero_shot.py (BASELINE configs[0]: the reference's own CPU-runnable case).

Kept from the reference: the command line (:31-72), adapter loading by parameter NAME from a fine-tune checkpoint
(`mona_state_dict` / `lora_state_dict` wrapper or a bare dict, :107-147 — names are the checkpoint wire format), eval mode,
the scoring rule (:176-222): logits[b, c] = mean over the class's prompts of 100 · <normalised image feature, normalised prompt
feature>, and the report (:224-290): Acc / Rec / Pre / F1 / AUC, the ROC curve and results.csv in a <time>_acc=<acc> folder.
The loop, the scoring kernel and the report are src/models/zero_shot_eval.py's, shared with the MetaCLIP, CLIP and UniMed-CLIP
entries; this module keeps the flags and the model.  The prompt ensembles are the reference's (src/models/zero_shot_prompt.py:29-54,
carried as data: ten prompts per class, picked by --dataset as in reference :168-173); --prompts_json overrides them.
Data: --synthetic or --data_pt {"images","labels"}.
"""
import argparse
import logging
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.adapters import inject_lora_to_biomedclip, inject_mona_variant_to_open_clip
from src.adapters.checkpoint import load_adapter_by_name
from src.models import zero_shot_eval as ZS
from src.models.zero_shot_prompt import ensemble_for  # noqa: F401  (the ensembles are part of this module's surface)
from src.third_party.biomedclip.model import SyntheticTokenizer, create_biomedclip
from src.utils.tools import parse_config

LESION_TYPES = ("benign", "malignant")


def get_args(argv=None):
    p = argparse.ArgumentParser("Adaptation of Visual Foundation Model for Medical Ultrasound Image Analysis")
    p.add_argument("--exp", type=str, default="biomedclip_zero_shot")
    p.add_argument("--dataset", type=str, default="LN-INT")
    p.add_argument("--img_size", type=int, default=224)
    p.add_argument("--patch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=False, action=argparse.BooleanOptionalAction)
    p.add_argument("--weak_augs", default=False, action=argparse.BooleanOptionalAction)
    p.add_argument("--mona_weights", type=str, default=None)
    p.add_argument("--mona_variant", type=str, default="freq_enhanced", choices=["baseline", "fractional", "noise_aware", "freq_enhanced", "hybrid"])
    p.add_argument("--mona_bottleneck", type=int, default=64)
    p.add_argument("--mona_layers", type=int, default=None)
    p.add_argument("--lora_weights", type=str, default=None)
    p.add_argument("--lora_r", type=int, default=16)
    p.add_argument("--lora_alpha", type=int, default=32)
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--device", type=str, default="cuda:0" if torch.cuda.is_available() else "cpu")
    # additions of this build
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--synthetic_test", type=int, default=64)
    p.add_argument("--data_pt", type=str, default=None, help=".pt with {'images': [N,3,S,S], 'labels': [N]}")
    p.add_argument("--data_root", type=str, default=None, help="refused here: the folder loader serves the supervised classification / segmentation entries")
    p.add_argument("--prompts_json", type=str, default=None, help='{"benign": [...], "malignant": [...]}')
    p.add_argument("--ckpt_path", type=str, default=None)
    p.add_argument("--model_config", type=str, default=None)
    return p.parse_args(argv)


def prepare_model(args):
    cfg = parse_config(args.model_config) if args.model_config else None
    state = torch.load(args.ckpt_path, map_location="cpu") if args.ckpt_path else None
    model = create_biomedclip(state_dict=state, config=cfg, seed=args.seed)
    tokenizer = SyntheticTokenizer(256 if cfg is None else cfg["text_cfg"]["max_position_embeddings"])
    if args.lora_weights:
        inject_lora_to_biomedclip(model, lora_r=args.lora_r, lora_alpha=args.lora_alpha, lora_dropout=0.0)
        n = load_adapter_by_name(model, args.lora_weights, "lora_state_dict")
        logging.info(f"✓ Loaded {n} LoRA parameters from {args.lora_weights}")
    elif args.mona_weights:
        inject_mona_variant_to_open_clip(model, variant=args.mona_variant, bottleneck_dim=args.mona_bottleneck, num_layers=args.mona_layers)
        n = load_adapter_by_name(model, args.mona_weights, "mona_state_dict")
        logging.info(f"✓ Loaded {n} MONA parameters from {args.mona_weights}")
    for p in model.parameters():
        p.requires_grad = False
    model.float()
    model.to(args.device)
    model.eval()
    return model, tokenizer


def _test_batches(args):
    images, labels = ZS.load_test_split(args)
    for i in range(0, len(labels), args.batch_size):
        yield images[i:i + args.batch_size], labels[i:i + args.batch_size]


@torch.no_grad()
def test(args):
    """-> (stats: acc / rec / pre / f1 / auc / loss / n, logits [N, 2] on the host)."""
    stats, logits, _ = ZS.run(args, "biomedclip", prepare_model)
    return stats, logits.cpu()


def main(argv=None):
    return ZS.main(get_args(argv), "biomedclip", prepare_model)


if __name__ == "__main__":
    main()
