"""MetaCLIP zero-shot classification on the MI355X HIP path — counterpart of /root/reference/src/models/metaclip/zero_shot.py; the evaluation that
src/models/metaclip/finetune.py --zero_shot_eval starts after training.

Same command line (every flag and default of reference :34-58) and model preparation (:88-113): the MetaCLIP model as finetune.py here builds it
(create_metaclip: --ckpt_path or a seeded random init), Mona adapters injected when --mona_weights is given and the checkpoint — the bare dict of "mona"
parameters that finetune.py saves — loaded with strict=False, eval mode.  The loop, the scoring kernel and the report are src/models/zero_shot_eval.py's.
Added, as in the BiomedCLIP entry: --dtype, --synthetic, --synthetic_test, --data_pt, --prompts_json, --ckpt_path, --model_config.  Prompts are tokenised
by the deterministic stand-in tokenizer of the fine-tune entry."""
import argparse
import logging
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.adapters import inject_mona_variant_to_open_clip
from src.models import zero_shot_eval as ZS
from src.models.metaclip.finetune import make_tokenizer
from src.third_party.open_clip.model import create_metaclip
from src.utils.tools import default_device, parse_config
from uia_hip import functional as UF


def get_args(argv=None):
    p = argparse.ArgumentParser("Zero-shot Classification with MetaCLIP")
    p.add_argument("--exp", type=str, default="metaclip_zero_shot")
    p.add_argument("--dataset", type=str, default="LN-INT")
    p.add_argument("--img_size", type=int, default=224)
    p.add_argument("--num_workers", type=int, default=8)
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


def load_mona_non_strict(model, path):
    """reference :101-109: the checkpoint IS the state dict of the "mona" parameters; strict=False."""
    model.load_state_dict(torch.load(path, map_location="cpu", weights_only=True), strict=False)
    UF.WEIGHTS.bump()                                   # operand copies of the replaced weights are stale


def prepare_model(args):
    cfg = parse_config(args.model_config) if args.model_config else None
    state = torch.load(args.ckpt_path, map_location="cpu") if args.ckpt_path else None
    model = create_metaclip(state_dict=state, config=cfg, seed=args.seed)
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
    stats, logits, _ = ZS.run(args, "metaclip", prepare_model)
    return stats, logits.cpu()


def main(argv=None):
    return ZS.main(get_args(argv), "metaclip", prepare_model)


if __name__ == "__main__":
    main()
