"""The host-side rule that picks the split count of the extend attention (models/generation.py,
``_extend_splits``)."""
import pytest

from distributed_pytorch_from_scratch_amd.models.generation import _extend_splits


@pytest.mark.parametrize("env,T,B,h,t_max,cus,want", [
    ("auto", 256, 8, 12, 32768, 256, 1),       # 768 workgroups already: a full grid
    ("auto", 32, 1, 12, 1024, 256, 1),         # 32 key tiles: under MIN_TILES per split at 2 splits
    ("auto", 32, 1, 12, 2016, 256, 1),         # 63 tiles: the last capacity that never splits
    ("auto", 32, 1, 12, 2017, 256, 2),
    ("auto", 8, 8, 32, 32768, 256, 1),         # one workgroup per CU already
    ("auto", 32, 1, 12, 16384, 256, 16),       # 512 tiles // 32, below 256 // 12 = 21
    ("auto", 33, 1, 32, 32768, 256, 4),        # 64 workgroups: 256 // 64, below 1024 // 32
    ("auto", 8, 1, 1, 1 << 20, 256, 64),       # capped
    ("0", 8, 1, 1, 1 << 20, 256, 1), ("5", 256, 8, 12, 128, 256, 5), ("200", 8, 1, 1, 64, 256, 64),
])
def test_extend_splits_rule(monkeypatch, env, T, B, h, t_max, cus, want):
    monkeypatch.setenv("DPFS_EXTEND_SPLIT", env)
    assert _extend_splits(T, B, h, t_max, cus) == want
