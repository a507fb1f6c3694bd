"""The signatures of the paged KV cache bindings of ``_C`` against their recorded form
(``tests/golden/ext_api_paged.txt``).  ``tests/test_ext_api.py`` records the public names of the
extension only and its golden file stays as it is, so the four paged launches are bound with
leading underscores and recorded here: a renamed argument, a changed order or a lost default in
``csrc/bindings/decode.cpp`` fails this test; an intended change re-records the file
(``python tests/test_ext_api_paged.py``)."""
import glob
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ext_api_paged.txt")
NAMES = ["_attn_decode_paged", "_rope_append_paged", "_kv_append_chunk_paged", "_attn_extend_paged"]


def dump(mod) -> str:
    return "".join(f"== {n}\n{(getattr(mod, n).__doc__ or '').strip()}\n" for n in NAMES)


def _built() -> bool:
    return bool(glob.glob(os.path.join(ROOT, "distributed_pytorch_from_scratch_amd", "_C.*.so")))


@pytest.mark.skipif(not _built(), reason="the native extension is not built")
def test_paged_bindings_match_golden():
    import torch  # noqa: F401  (the extension links against it)
    mod = importlib.import_module("distributed_pytorch_from_scratch_amd._C")
    for n in NAMES:
        assert hasattr(mod, n) and not hasattr(mod, n[1:])        # one binding each, under this name
    with open(GOLDEN) as f:
        want = f.read()
    assert dump(mod) == want
    # every one: the pools, the optional scale pools, the table, the lengths, ..., t_max and the page size
    for block in want.split("== ")[1:]:
        order = ["k_pool: torch.Tensor", "v_pool: torch.Tensor", "ks: torch.Tensor | None", "vs: torch.Tensor | None",
                 "tbl: torch.Tensor", "len: torch.Tensor", "t_max:", "page:"]
        at = [block.index(s) for s in order]
        assert at == sorted(at)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    with open(GOLDEN, "w") as f:
        f.write(dump(importlib.import_module("distributed_pytorch_from_scratch_amd._C")))
    print("wrote", GOLDEN)
