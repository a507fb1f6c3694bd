"""The signature and docstring of ``_C._sample_logits_pen`` against their recorded form
(``tests/golden/ext_api_sample_pen.txt``).  ``tests/test_ext_api.py`` records the public names of
the extension only and its golden file stays as it is, as does the per-row form's
(``tests/golden/ext_api_sample_rows.txt``), so the penalised sampling launch is bound with a
leading underscore and recorded here: a renamed argument, a dropped default or a lost docstring
in ``csrc/bindings/decode.cpp`` fails this test; an intended change re-records the file
(``python tests/test_ext_api_sample_pen.py``)."""
import glob
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ext_api_sample_pen.txt")
NAME = "_sample_logits_pen"


def dump(mod) -> str:
    return f"== {NAME}\n{(getattr(mod, NAME).__doc__ or '').strip()}\n"


def _built() -> bool:
    return bool(glob.glob(os.path.join(ROOT, "distributed_pytorch_from_scratch_amd", "_C.*.so")))


@pytest.mark.skipif(not _built(), reason="the native extension is not built")
def test_sample_logits_pen_binding_matches_golden():
    import torch  # noqa: F401  (the extension links against it)
    mod = importlib.import_module("distributed_pytorch_from_scratch_amd._C")
    assert hasattr(mod, NAME) and not hasattr(mod, NAME[1:])      # one binding, under this name
    with open(GOLDEN) as f:
        want = f.read()
    assert dump(mod) == want
    # the per-row form's arguments, then the penalties and the history, then pos / u / update
    order = ["logits:", "vocab:", "inv_t:", "top_k:", "top_p:", "seed:", "rid:", "rep:", "inv_rep:", "pres:", "freq:",
             "hist: torch.Tensor", "pos:", "u: torch.Tensor | None = None", "update: bool = True", "-> tuple"]
    at = [want.index(s) for s in order]
    assert at == sorted(at)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    with open(GOLDEN, "w") as f:
        f.write(dump(importlib.import_module("distributed_pytorch_from_scratch_amd._C")))
    print("wrote", GOLDEN)
