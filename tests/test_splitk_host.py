"""Low-latency fp32 plans, host side (no GPU): the split-K heuristic y3_choose_split_k, the Python argument checks and the
`low_latency` key of Inference."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256


def _choose(tiles, k_tiles, n_cus=CUS, slab=1 << 16):
    from yolo_v3_tf2_amd import _lib
    return _lib.load().y3_choose_split_k(tiles, k_tiles, n_cus, slab)


def _slab(M, cout_pad, bm=64):
    return -(-M // bm) * bm * cout_pad * 4


def test_no_split_once_the_tiles_fill_the_chip():
    for tiles in (2 * CUS, 2 * CUS + 1, 1024, 100000):
        for kt in (4, 18, 144):
            assert _choose(tiles, kt) == 1
    assert _choose(2 * CUS - 1, 144) == 2
    # degenerate arguments: the ordinary launch
    assert _choose(0, 144) == 1 and _choose(48, 0) == 1 and _choose(48, 144, 0) == 1 and _choose(48, 144, CUS, 0) == 1


def test_caps_k_tiles_sixteen_and_slab_bytes():
    for tiles in range(1, 2 * CUS, 7):
        for kt in (1, 3, 4, 7, 8, 12, 18, 36, 72, 144, 1000):
            for slab in (1 << 10, 1 << 20, 3 << 20, 5 << 20, 9 << 20, 17 << 20):
                S = _choose(tiles, kt, CUS, slab)
                assert 1 <= S <= 16
                assert S == 1 or (S <= kt // 4 and S * slab <= 16 << 20)
                # the smallest S that reaches two workgroups per CU, unless a cap stops it earlier
                assert S == 1 or tiles * (S - 1) < 2 * CUS
    assert _choose(1, 1000) == 16                 # the cap of 16
    assert _choose(24, 32) == 8                   # k_tiles / 4
    assert _choose(24, 7) == 1                    # k_tiles / 4 < 2
    assert _choose(24, 144, CUS, 4 << 20) == 4    # 16 MiB of slabs
    assert _choose(24, 144, CUS, 9 << 20) == 1


def test_monotone_in_tiles():
    for kt in (8, 18, 36, 144):
        for slab in (1 << 16, 3 << 20):
            prev = None
            for tiles in range(1, 2 * CUS + 10):
                S = _choose(tiles, kt, CUS, slab)
                assert prev is None or S <= prev, (tiles, kt, slab)
                prev = S


# Darknet-53 + necks at one 416^2 image on 256 CUs.  No tile reaches the 1024 workgroups choose_tile asks for, so every conv
# below runs the 64x64 tile (id 11): tiles = ceil(M / 64) * Cout / 64, k_tiles = K / 32, slab = ceil(M / 64) * 64 * Cout * 4.
# S = min(ceil(512 / tiles), k_tiles // 4, 16, 16 MiB // slab), and 1 where that is below 2.  Worked out by hand:
#   (grid, ksize, Cin, Cout, expected S)
DARKNET_B1_416 = [
    (104, 3, 64, 128, 2),      # 338 tiles -> 2
    (104, 1, 128, 64, 1),      # 169 tiles -> 4 wanted, but 4 K tiles: k_tiles // 4 = 1
    (52, 3, 128, 256, 3),      # 43 * 4 = 172 tiles -> 3
    (52, 1, 256, 128, 2),      # 86 tiles -> 6 wanted, 8 K tiles -> 2
    (52, 1, 384, 128, 3),      # the neck's concat 1x1: 86 tiles -> 6 wanted, 12 K tiles -> 3
    (26, 3, 256, 512, 6),      # 11 * 8 = 88 tiles -> 6
    (26, 1, 512, 256, 4),      # 44 tiles -> 12 wanted, 16 K tiles -> 4
    (26, 1, 768, 256, 6),      # concat 1x1: 24 K tiles -> 6
    (13, 3, 512, 1024, 11),    # 3 * 16 = 48 tiles -> 11
    (13, 1, 1024, 512, 8),     # 24 tiles -> 22 wanted, 32 K tiles -> 8
]


@pytest.mark.parametrize("grid,k,cin,cout,want", DARKNET_B1_416)
def test_darknet53_batch1_416_values(grid, k, cin, cout, want):
    M = grid * grid
    tiles = -(-M // 64) * (cout // 64)
    assert _choose(tiles, k * k * cin // 32, CUS, _slab(M, cout)) == want


def test_darknet53_batch64_never_splits():
    for grid, k, cin, cout, _ in DARKNET_B1_416:
        M = 64 * grid * grid
        assert _choose(-(-M // 64) * (cout // 64), k * k * cin // 32, CUS, _slab(M, cout)) == 1


def test_python_argument_checks():
    """The checks run before the library is touched, so an object without a device net shows them."""
    from yolo_v3_tf2_amd import runtime
    Net, Y3Error = runtime.Net, runtime.Y3Error
    assert Net._low_latency_arg(None) is False and Net._low_latency_arg(False) is False
    assert Net._low_latency_arg(True) is True and Net._low_latency_arg(1) is True and Net._low_latency_arg(np.bool_(True)) is True
    for bad in (2, -1, "yes", 1.0, [True]):
        with pytest.raises(Y3Error, match="low_latency"):
            Net._low_latency_arg(bad)
    for ok in (-1, 1, 2, 9, 16, np.int64(4)):
        assert Net._split_k_arg(ok) == int(ok)
    for bad in (0, -2, 17, 2.0, "4", None, True):
        with pytest.raises(Y3Error, match="split_k"):
            Net._split_k_arg(bad)
    net = Net.__new__(Net)          # no device object: every call below must raise before it would need one
    net.conv_ops = [object()] * 3
    net._h = None
    with pytest.raises(Y3Error, match="split_k"):
        net.set_split_k(0, 0)
    for bad_slot in (-1, 3, 1.0, None, True):
        with pytest.raises(Y3Error, match="conv slot"):
            net.set_split_k(bad_slot, 2)
        with pytest.raises(Y3Error, match="conv slot"):
            net.split_k(bad_slot)
    with pytest.raises(Y3Error, match="low_latency"):
        net.set_low_latency("on")


def test_model_remembers_low_latency_until_the_device_net_exists(program):
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    from yolo_v3_tf2_amd.runtime import Y3Error
    m = YoloModel(program)
    assert m.low_latency is False
    m.set_low_latency(True)
    assert m.low_latency is True and m._net is None
    m.set_low_latency(None)
    assert m.low_latency is False
    with pytest.raises(Y3Error):
        m.set_low_latency(3)


@pytest.mark.parametrize("value,want", [(None, False), (False, False), (True, True)])
def test_inference_build_accepts_and_forwards_the_key(weights, tmp_path, monkeypatch, value, want):
    import inspect
    import yaml
    from yolo_v3_tf2_amd.inference import Inference
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config/detect_config_coco.yaml")))
    assert cfg.get("low_latency", None) is None                       # the packaged config leaves it off; a YAML without the key works too
    assert inspect.signature(Inference.__call__).parameters["low_latency"].default is None
    monkeypatch.chdir(tmp_path)                                       # build() writes model_inference_summary.txt
    kw = {} if value is None else {"low_latency": value}
    model, names = Inference().build(os.path.join(ROOT, cfg["model_config_file"]), os.path.join(ROOT, cfg["classes_name_file"]),
                                     os.path.join(ROOT, cfg["anchors_file"]), None, 100, 0.5, 0.1, weights=weights, **kw)
    assert len(names) == 80 and model.model.low_latency is want and model.model._net is None
    with pytest.raises(Exception, match="low_latency"):
        Inference().build(os.path.join(ROOT, cfg["model_config_file"]), os.path.join(ROOT, cfg["classes_name_file"]),
                          os.path.join(ROOT, cfg["anchors_file"]), None, 100, 0.5, 0.1, weights=weights, low_latency="fast")
