"""What tests/golden/moe_pass_bits.json pins, shared by its recorder (tools/record_moe_bits.py) and tests/test_engine_moe_gemm_gpu.py: the engine passes over the
four models of tests/moe_ref.py whose logits must stay the bits of the build BEFORE the grouped expert GEMM -- every pass with moe_gemm = 0, and the one-row
passes (a 1-token prompt, fused decode steps) at any setting.  One SHA-256 per (model, pass) over the float32 logits.

Passes of one engine, in this order (the KV cache carries over where a pass starts behind another):
  p1 / p3 / p4 / p37 / p70   a prompt of that many tokens at position 0
  chunk                      37 tokens at 0, then 33 at 37: the second pass's logits
  steps                      37 tokens at 0, then eight fused graph decode steps fed FED (fixed tokens, no oracle needed): all eight logit rows
"""
import hashlib
import os

import numpy as np

from moe_ref import MODELS, model_file, prompt_tokens

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moe_pass_bits.json")
PROMPTS = (1, 3, 4, 37, 70)
FED = (11, 200, 3, 77, 140, 9, 251, 64)
ONE_ROW = ("p1",)          # a pass that never takes the GEMM form (the steps too, but their KV cache comes from a 37-token pass that may)
NAMES = sorted(MODELS)


class TmpDirs:
    """what moe_ref.model_file needs of pytest's tmp_path_factory, for the recorder"""

    def __init__(self, root):
        self.root, self.n = root, 0

    def mktemp(self, name):
        import pathlib
        self.n += 1
        p = pathlib.Path(self.root) / ("%s%d" % (name, self.n))
        p.mkdir(parents=True)
        return p


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, np.float32)).tobytes()).hexdigest()


def run_passes(e, only=None):
    """{pass name: logits} of engine e (see the module docstring); only: a subset of the names"""
    toks = prompt_tokens()
    out = {}
    for T in PROMPTS:
        if only is None or "p%d" % T in only:
            out["p%d" % T] = e.forward(toks[:T], 0)
    if only is None or "chunk" in only:
        e.forward(toks[:37], 0)
        out["chunk"] = e.forward(toks[37:70], 37)
    if only is None or "steps" in only:
        e.forward(toks[:37], 0)
        out["steps"] = np.stack([e.decode_fused(tok, 37 + i, graph=True) for i, tok in enumerate(FED)])
    return out


def model_path(name, tmp_path_factory):
    return model_file(name, tmp_path_factory)
