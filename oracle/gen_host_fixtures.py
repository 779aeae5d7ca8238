"""Writes the data fixtures of two host tests (tests/test_round6_host.py), so that they run without the reference tree:

    python oracle/gen_host_fixtures.py REFERENCE_DIR     (REFERENCE_DIR: a checkout of the reference project; only the data below is kept)

  tests/golden/reference_cli_tables.json   the argparse table of every reference entry point: flag -> {default / action / choices: source expression}
  tests/golden/bpe_prompt_case.json        the four CLIPSeg prompt strings (reference src/models/clipseg/prompt.py) and the merge rules of the reference's
                                           merges file that FIRE while oracle/bpe_ref.py tokenises the texts the test tokenises, each with its line number.
                                           Greedy BPE fuses the lowest-ranked pair present; every pair it fuses is in the subset with its own rank, so a merges
                                           file holding only these rules at their own lines (inert fillers elsewhere) yields the same tokens and the same ids.
"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = ["biomedclip/finetune.py", "biomedclip/segmentation.py", "biomedclip/zero_shot.py", "clipseg/segmentation.py", "metaclip/finetune.py",
           "clip/finetune.py", "unimedclip/finetune.py"]
# the texts tests/test_round6_host.py::test_bpe_restatement_reproduces_the_committed_ids tokenises besides the four prompts
EXTRA_TEXTS = ["a photo of a cat", "breast lesion " * 60]


def argparse_table(path):
    import ast
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument" and node.args and isinstance(node.args[0], ast.Constant):
            out[node.args[0].value] = {k.arg: ast.unparse(k.value) for k in node.keywords if k.arg in ("default", "action", "choices")}
    return out


def fired_rules(bpe, texts):
    """{rank: [a, b]} of every rule bpe.merge() applies while encoding `texts`."""
    used = {}
    rank = bpe.rank
    orig = bpe.merge

    def merge(token):
        parts = list(token[:-1]) + [token[-1] + "</w>"]
        out = orig(token)
        # replay: the rules applied are the adjacent pairs fused on the way from `parts` to `out`
        while len(parts) > 1:
            best = min(((rank[(a, b)], k) for k, (a, b) in enumerate(zip(parts, parts[1:])) if (a, b) in rank), default=None)
            if best is None:
                break
            a, b = parts[best[1]], parts[best[1] + 1]
            used[best[0]] = [a, b]
            nxt, k = [], 0
            while k < len(parts):
                if k + 1 < len(parts) and parts[k] == a and parts[k + 1] == b:
                    nxt.append(a + b)
                    k += 2
                else:
                    nxt.append(parts[k])
                    k += 1
            parts = nxt
        assert parts == out, (token, parts, out)
        return out

    bpe.merge = merge
    for t in texts:
        bpe.encode(t)
    bpe.merge = orig
    return used


def main(ref):
    from oracle.bpe_ref import BPE
    from oracle import gen_prompt_ids
    tables = {e: argparse_table(os.path.join(ref, "src/models", e)) for e in ENTRIES}
    assert all(tables.values())
    with open(os.path.join(GOLDEN, "reference_cli_tables.json"), "w") as f:
        json.dump(tables, f, indent=1, sort_keys=True)
    gen_prompt_ids.REF = ref                                   # prompt_strings() reads the reference's prompt.py under gen_prompt_ids.REF
    prompts = gen_prompt_ids.prompt_strings()
    bpe = BPE(os.path.join(ref, "src/third_party/openai_clip/bpe_simple_vocab_16e6.txt.gz"))
    used = fired_rules(bpe, list(prompts.values()) + EXTRA_TEXTS)
    case = {"prompts": prompts, "merges": {str(r): used[r] for r in sorted(used)}}
    with open(os.path.join(GOLDEN, "bpe_prompt_case.json"), "w") as f:
        json.dump(case, f, indent=1)
    print(f"{len(tables)} CLI tables, {len(prompts)} prompts, {len(used)} merge rules")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python oracle/gen_host_fixtures.py REFERENCE_DIR")
    main(sys.argv[1])
