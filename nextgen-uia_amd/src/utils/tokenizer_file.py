"""`--tokenizer_json FILE`: real token ids from a tokenizer file of the `tokenizers` library (the tokenizer.json beside a released checkpoint),
in place of the stand-in tokenizers, which hash words into ids.  Truncation and padding are set to the family's context length and pad id through
the library's own calls, so the file's post-processor keeps its start / end tokens when a caption is cut.  No vocabulary is shipped."""
import os

import torch

PROBE = "a probe caption of several common words"


class FileTokenizer:
    """texts -> int64 [n, context_length], the call the stand-in tokenizers answer."""

    def __init__(self, path, context_length, pad_id=0):
        try:
            from tokenizers import Tokenizer
        except ImportError as e:
            raise RuntimeError("--tokenizer_json needs the `tokenizers` library, which is not installed") from e
        os.environ.setdefault("TOKENIZERS_PARALLELISM", "false")       # the loader workers are forked and tokenise there: no thread pool of the library's own
        self.path, self.context_length, self.pad_id = str(path), int(context_length), int(pad_id)
        self.tk = Tokenizer.from_file(self.path)
        self.tk.enable_truncation(max_length=self.context_length)
        self.tk.enable_padding(length=self.context_length, pad_id=self.pad_id, pad_token=self.tk.id_to_token(self.pad_id) or "[PAD]")

    def __call__(self, texts):
        if isinstance(texts, str):
            texts = [texts]
        return torch.tensor([e.ids for e in self.tk.encode_batch(list(texts))], dtype=torch.long).reshape(len(texts), self.context_length)

    def largest_id(self):
        return max(self.tk.get_vocab(with_added_tokens=True).values())

    def check(self, table_rows, pools_at_argmax):
        """Start-up refusals, before any launch.  table_rows: rows of the text tower's embedding table — an id beyond it would be read out of bounds on
        the device.  pools_at_argmax: the CLIP-layout towers take the features at the arg-max id of a caption, which must be the end token."""
        if self.largest_id() >= int(table_rows):
            raise RuntimeError(f"--tokenizer_json {self.path}: the vocabulary reaches id {self.largest_id()}, the text tower's embedding table has {table_rows} rows")
        if pools_at_argmax:
            enc = self.tk.encode(PROBE)
            real = [i for i, m in zip(enc.ids, enc.attention_mask) if m]
            if not real or real[-1] != max(real) or real.count(real[-1]) != 1:
                raise RuntimeError(f"--tokenizer_json {self.path}: the text tower pools at the arg-max token id, so the end token must be the largest id of a "
                                   f"caption; the probe {PROBE!r} encodes to {real}")
        return self


def from_args(args, context_length, table_rows, pools_at_argmax, pad_id=0):
    """The families' make_tokenizer: the checked FileTokenizer of --tokenizer_json, or None without the flag (the stand-in stays)."""
    path = getattr(args, "tokenizer_json", None)
    if not path:
        return None
    return FileTokenizer(path, context_length, pad_id).check(table_rows, pools_at_argmax)
