"""OpenAI-CLIP zero-shot classification on the MI355X HIP path — counterpart of /root/reference/src/models/clip/zero_shot.py; the evaluation that
src/models/clip/finetune.py --zero_shot_eval starts after training.

Same command line (every flag and default of reference :43-79; the augmentation, --reduce_dim and LoRA flags are carried although the reference's
prepare_model reads none of them) and model preparation (:110-142): the OpenAI-layout CLIP as finetune.py here loads it (load_clip: --ckpt, or
--ckpt_path when given, as a TorchScript archive or a state dict, else a seeded random init), fp32, Mona adapters injected when --mona_weights is given
and the checkpoint's tensors copied BY NAME into the model's state dict — at least one must match — as the reference file has it, eval mode.  The loop,
the scoring kernel and the report are src/models/zero_shot_eval.py's.  Added, as in the BiomedCLIP entry: --dtype, --synthetic, --synthetic_test,
--data_pt, --prompts_json, --ckpt_path, --model_config.  Prompts are tokenised by the deterministic stand-in tokenizer of the fine-tune entry."""
import argparse
import logging
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.adapters import inject_mona_variant_to_clip
from src.adapters.checkpoint import load_adapter_by_name
from src.models import zero_shot_eval as ZS
from src.models.clip.finetune import _geometry, make_tokenizer
from src.third_party.openai_clip.model import load_clip
from src.utils.tools import default_device


def get_args(argv=None):
    p = argparse.ArgumentParser("Adaptation of Visual Foundation Model for Medical Ultrasound Image Analysis")
    p.add_argument("--exp", type=str, default="clip_zero_shot")
    p.add_argument("--dataset", type=str, default="LN-INT")
    p.add_argument("--img_size", type=int, default=224)
    p.add_argument("--patch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=True, action=argparse.BooleanOptionalAction)
    p.add_argument("--weak_augs", default=True, action=argparse.BooleanOptionalAction)
    p.add_argument("--ckpt", type=str, default="ckpt/ViT-B-16.pt")
    p.add_argument("--mona_variant", type=str, default="noise_aware")
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
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--device", type=str, default=default_device())
    ZS.add_build_flags(p)
    return p.parse_args(argv)


def prepare_model(args):
    logging.info("Loading CLIP model")
    model = load_clip(args.ckpt_path or args.ckpt, _geometry(args), args.seed)
    model.float()
    if args.mona_weights:
        model, mona_count = inject_mona_variant_to_clip(model, variant=args.mona_variant, bottleneck_dim=args.mona_bottleneck, num_layers=args.mona_layers)
        n = load_adapter_by_name(model, args.mona_weights)       # reference :125-139: a bare dict of tensors, no wrapper key
        logging.info(f"✓ Loaded {n} pretrained MONA parameters from {args.mona_weights}")
    for p in model.parameters():
        p.requires_grad = False
    model.to(args.device)
    model.eval()
    return model, make_tokenizer(args)


@torch.no_grad()
def test(args):
    """-> (stats: acc / rec / pre / f1 / auc / loss / n, logits [N, 2] on the host)."""
    stats, logits, _ = ZS.run(args, "clip", prepare_model)
    return stats, logits.cpu()


def main(argv=None):
    return ZS.main(get_args(argv), "clip", prepare_model)


if __name__ == "__main__":
    main()
