"""Loading a fine-tune checkpoint's adapter tensors into a model whose adapters have been injected."""
import torch

from uia_hip import functional as UF


def load_adapter_by_name(model, path, wrapper_key=None):
    """reference biomedclip/zero_shot.py:107-119 / :136-147, clip/zero_shot.py:125-139: copy every checkpoint tensor whose name exists in the model (names are the
    checkpoint wire format); at least one must.  wrapper_key: the checkpoint may hold its tensors under this key (`mona_state_dict` / `lora_state_dict`) or bare."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if wrapper_key is not None:
        state = state.get(wrapper_key, state)
    model_dict = model.state_dict()
    loaded = 0
    for name, param in state.items():
        if name in model_dict:
            model_dict[name] = param
            loaded += 1
    assert loaded > 0, f"No adapter parameters loaded from {path}"
    model.load_state_dict(model_dict)
    UF.WEIGHTS.bump()                                   # operand copies of the replaced weights are stale
    return loaded
