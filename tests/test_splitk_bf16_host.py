"""Low-latency bf16 plans without a GPU: the number of K slices y3_choose_split_k gives each eligible conv shape of a bf16 plan for one
416 x 416 image, and the three entry points in the header and the binding.

The inputs are the ones resolve_splits feeds the rule for a bf16 plan: workgroups of the 64x64 LDS-DMA tile (id 11, where
choose_tile_bf16 ends for every conv that cannot reach 512 workgroups), K tiles of 64, 256 compute units, the bytes of one fp32 slab
[Mpad][CoutPad]."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (ksize, Cin, Cout, grid side) -> (workgroups, K tiles, slab bytes, S of the rule, S in force): pinned literals.  In force: the rule's S for a
# conv of at least 32 K tiles, else 1 (kSplitMinKTilesBf16 in csrc/y3_net.cpp, set from profiles/latency_bf16_splitk_sweep.txt); the library
# is held to that column on the GPU (tests/test_splitk_bf16_gpu.py::test_low_latency_bf16_plan_follows_the_pinned_table)
RULE_B1_S416 = [
    ((3, 512, 1024, 13), (48, 72, 786432, 11, 11)),
    ((1, 1024, 512, 13), (24, 16, 393216, 4, 1)),
    ((3, 256, 512, 26), (88, 36, 1441792, 6, 6)),
    ((1, 512, 256, 26), (44, 8, 720896, 2, 1)),
    ((1, 768, 256, 26), (44, 12, 720896, 3, 1)),      # the neck's up-sample + concat 1x1
    ((3, 128, 256, 52), (172, 18, 2818048, 3, 1)),
    ((1, 256, 128, 52), (86, 4, 1409024, 1, 1)),      # 4 K tiles: one slice of at least 4 tiles is the unsplit launch
    ((1, 384, 128, 52), (86, 6, 1409024, 1, 1)),
]


@pytest.mark.parametrize("shape,want", RULE_B1_S416)
def test_rule_for_one_416_image(shape, want):
    from yolo_v3_tf2_amd import _lib
    k, cin, cout, g = shape
    M = g * g
    tiles = -(-M // 64) * (cout // 64)
    k_tiles = k * k * cin // 64
    slab = -(-M // 64) * 64 * cout * 4
    assert (tiles, k_tiles, slab) == want[:3]
    assert _lib.load().y3_choose_split_k(tiles, k_tiles, 256, slab) == want[3]
    assert want[4] == (want[3] if k_tiles >= 32 else 1)      # the table's own two columns agree with the threshold as documented


def test_entry_points_are_declared_and_bound():
    from yolo_v3_tf2_amd import _lib, runtime
    header = open(os.path.join(ROOT, "include", "y3.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in ("y3_net_set_low_latency_bf16", "y3_net_set_split_k_bf16", "y3_net_get_split_k_bf16"):
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("set_low_latency_bf16", "set_split_k_bf16", "split_k_bf16"):
        assert callable(getattr(runtime.Net, name)), name
