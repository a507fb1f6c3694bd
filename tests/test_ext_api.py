"""The Python-visible surface of the native extension ``_C`` against its recorded form
(``tests/golden/ext_api.txt``): every public name with its pybind11 docstring, which holds the
full signature (argument names, types, defaults) and the help text.  A rename, a dropped default
or a lost docstring in ``csrc/bindings/`` fails here; an intended change re-records the file
(``python tests/test_ext_api.py``)."""
import glob
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ext_api.txt")


def dump_api(mod) -> str:
    out = []
    for name in sorted(n for n in dir(mod) if not n.startswith("_")):
        out.append(f"== {name}\n{(getattr(mod, name).__doc__ or '').strip()}\n")
    return "\n".join(out)


def _built() -> bool:
    return bool(glob.glob(os.path.join(ROOT, "distributed_pytorch_from_scratch_amd", "_C.*.so")))


@pytest.mark.skipif(not _built(), reason="the native extension is not built")
def test_ext_api_matches_golden():
    import torch  # noqa: F401  (the extension links against it)
    mod = importlib.import_module("distributed_pytorch_from_scratch_amd._C")
    with open(GOLDEN) as f:
        want = f.read()
    got = dump_api(mod)
    if got != want:
        import difflib
        diff = "\n".join(difflib.unified_diff(want.splitlines(), got.splitlines(), "golden", "built", lineterm="", n=1))
        pytest.fail("the _C module surface differs from tests/golden/ext_api.txt:\n" + diff[:6000])


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    with open(GOLDEN, "w") as f:
        f.write(dump_api(importlib.import_module("distributed_pytorch_from_scratch_amd._C")))
    print("wrote", GOLDEN)
