"""FocalLoss with MONAI 1.5.1 semantics (reference: src/models/*/classification.py:77, `FocalLoss(to_onehot_y=True)`).

MONAI cannot be imported in this build, so the arithmetic below is restated from MONAI 1.5.1's `sigmoid_focal_loss` and `FocalLoss.forward`
(mean reduction) and is **unpinned**: for a target t = one_hot(label) and a logit x, element-wise
    bce = x - x·t - logsigmoid(x),  loss = exp(γ·logsigmoid(-x·(2t-1))) · bce,  × (t·α + (1-t)(1-α)) when alpha is set,
then the mean over all N·C elements.  The loss runs fused on the device (`uia_focal_fwd_bwd`: loss and d loss / d logits in one call).
The supported subset is what the reference trains with: to_onehot_y=True, the sigmoid form, mean reduction, any gamma, alpha None or a float;
anything else raises NotImplementedError."""
import torch
import torch.nn as nn

from uia_hip import ops


class _FocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, label, gamma, alpha):
        loss, dl = ops.focal_fwd_bwd(logits.contiguous().float(), label, gamma, alpha)
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None, None, None


class FocalLoss(nn.Module):
    def __init__(self, include_background=True, to_onehot_y=False, gamma=2.0, alpha=None, weight=None, reduction="mean", use_softmax=False):
        super().__init__()
        if not include_background:
            raise NotImplementedError("FocalLoss: include_background=False is not part of this build")
        if not to_onehot_y:
            raise NotImplementedError("FocalLoss: only to_onehot_y=True (class-index labels) is part of this build")
        if weight is not None:
            raise NotImplementedError("FocalLoss: per-class weight is not part of this build")
        if reduction != "mean":
            raise NotImplementedError(f"FocalLoss: reduction={reduction!r}; only 'mean' is part of this build")
        if use_softmax:
            raise NotImplementedError("FocalLoss: only the sigmoid form (use_softmax=False) is part of this build")
        if alpha is not None and not (0.0 <= float(alpha) <= 1.0):
            raise ValueError(f"FocalLoss: alpha={alpha} must lie in [0, 1]")
        if float(gamma) < 0:
            raise ValueError(f"FocalLoss: gamma={gamma} must be >= 0")
        self.gamma = float(gamma)
        self.alpha = None if alpha is None else float(alpha)

    def forward(self, logits, label):
        """logits [N, C]; label [N] or [N, 1] class indices."""
        if logits.dim() != 2:
            raise NotImplementedError(f"FocalLoss: logits of shape {tuple(logits.shape)}; this build takes [N, C]")
        return _FocalFn.apply(logits, label.reshape(-1), self.gamma, self.alpha)
