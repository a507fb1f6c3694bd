"""The split extend-attention bindings of ``_C`` against ``tests/golden/ext_api_extend_split.txt`` (the
pattern of ``tests/test_ext_api_wq.py``); ``python tests/test_ext_api_extend_split.py`` re-records an
intended change."""
import glob
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ext_api_extend_split.txt")
NAMES = ["_attn_extend_split", "_attn_extend_split_paged"]


def dump(mod) -> str:
    return "".join(f"== {n}\n{(getattr(mod, n).__doc__ or '').strip()}\n" for n in NAMES)


@pytest.mark.skipif(not glob.glob(os.path.join(ROOT, "distributed_pytorch_from_scratch_amd", "_C.*.so")),
                    reason="the native extension is not built")
def test_extend_split_bindings_match_golden():
    import torch  # noqa: F401  (the extension links against it)
    mod = importlib.import_module("distributed_pytorch_from_scratch_amd._C")
    for n in NAMES:
        assert hasattr(mod, n) and not hasattr(mod, n[1:])        # one binding each, under this name
    with open(GOLDEN) as f:
        assert dump(mod) == f.read()


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    with open(GOLDEN, "w") as f:
        f.write(dump(importlib.import_module("distributed_pytorch_from_scratch_amd._C")))
    print("wrote", GOLDEN)
