"""The W8A8 bindings of ``_C`` against ``tests/golden/ext_api_w8a8.txt`` (the form of ``tests/test_ext_api_wq.py``)."""
import glob
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["_gemm_nt_w8a8", "_gemm_nt_w8a8_ok", "_swiglu_quant_w8_rows"]


@pytest.mark.skipif(not glob.glob(os.path.join(ROOT, "distributed_pytorch_from_scratch_amd", "_C.*.so")),
                    reason="the native extension is not built")
def test_w8a8_bindings_match_golden():
    import torch  # noqa: F401  (the extension links against it)
    mod = importlib.import_module("distributed_pytorch_from_scratch_amd._C")
    for n in NAMES:
        assert hasattr(mod, n) and not hasattr(mod, n[1:])        # one binding each, under this name
    with open(os.path.join(ROOT, "tests", "golden", "ext_api_w8a8.txt")) as f:
        assert "".join(f"== {n}\n{(getattr(mod, n).__doc__ or '').strip()}\n" for n in NAMES) == f.read()
