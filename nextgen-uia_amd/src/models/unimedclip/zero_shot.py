"""UniMed-CLIP zero-shot classification on the MI355X HIP path — counterpart of /root/reference/src/models/unimedclip/zero_shot.py; the evaluation that
src/models/unimedclip/finetune.py --zero_shot_eval starts after training.

Same command line (every flag and default of reference :36-60) and model preparation (:92-136): open_clip's native ViT-B/16 with QuickGELU forced as
finetune.py here builds it (create_native_clip), ONLY the `visual.*` keys and `logit_scale` of the checkpoint loaded (--ckpt, or --ckpt_path when given;
the text tower keeps its initialisation, as in the reference), Mona adapters injected when --mona_weights is given and the checkpoint — the bare dict of
"mona" parameters — loaded with strict=False, eval mode.  The loop, the scoring kernel and the report are src/models/zero_shot_eval.py's.  Added, as in the
BiomedCLIP entry: --dtype, --synthetic, --synthetic_test, --data_pt, --prompts_json, --ckpt_path, --model_config.  Prompts are tokenised by the
deterministic BERT-style stand-in tokenizer of the fine-tune entry."""
import argparse
import logging
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.adapters import inject_mona_variant_to_open_clip
from src.models import zero_shot_eval as ZS
from src.models.metaclip.zero_shot import load_mona_non_strict
from src.models.unimedclip.finetune import _config, make_tokenizer
from src.third_party.open_clip.model import create_native_clip
from src.utils.tools import default_device


def get_args(argv=None):
    p = argparse.ArgumentParser("Zero-shot Classification with UniMedCLIP")
    p.add_argument("--exp", type=str, default="unimedclip_zero_shot")
    p.add_argument("--dataset", type=str, default="LN-INT")
    p.add_argument("--img_size", type=int, default=224)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--version", type=str, default="ViT-B-16-quickgelu")
    p.add_argument("--ckpt", type=str, default="ckpt/unimed_clip_vit_b16.pt")
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--mona_variant", type=str, default="noise_aware")
    p.add_argument("--mona_weights", type=str, default=None)
    p.add_argument("--mona_bottleneck", type=int, default=64)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--device", type=str, default=default_device())
    ZS.add_build_flags(p)
    return p.parse_args(argv)


def prepare_model(args):
    model = create_native_clip(args.version, config=_config(args), seed=args.seed, force_quick_gelu=True)
    ckpt = args.ckpt_path or args.ckpt
    if ckpt and os.path.exists(ckpt):
        checkpoint = torch.load(ckpt, map_location="cpu", weights_only=False)
        state_dict = checkpoint["state_dict"] if "state_dict" in checkpoint else checkpoint
        state_dict = {k.replace("module.", ""): v for k, v in state_dict.items()}
        visual_state_dict = {k: v for k, v in state_dict.items() if k.startswith("visual.") or k == "logit_scale"}
        model.load_state_dict(visual_state_dict, strict=False)
        logging.info(f"loaded {len(visual_state_dict)} visual tensors from {ckpt}")
    else:
        logging.info(f"checkpoint {ckpt} not found: randomly initialised {args.version}")
    if args.mona_weights:
        logging.info(f"Loading fine-tuned MONA adapters from {args.mona_weights}...")
        model, mona_count = inject_mona_variant_to_open_clip(model, variant=args.mona_variant, bottleneck_dim=args.mona_bottleneck)
        load_mona_non_strict(model, args.mona_weights)
        logging.info(f"✓ Loaded MONA adapters ({mona_count} layers)")
    for p in model.parameters():
        p.requires_grad = False
    model.float()
    model.to(args.device)
    model.eval()
    return model, make_tokenizer(args)


@torch.no_grad()
def test(args):
    """-> (stats: acc / rec / pre / f1 / auc / loss / n, logits [N, 2] on the host)."""
    stats, logits, _ = ZS.run(args, "unimedclip", prepare_model)
    return stats, logits.cpu()


def main(argv=None):
    return ZS.main(get_args(argv), "unimedclip", prepare_model)


if __name__ == "__main__":
    main()
