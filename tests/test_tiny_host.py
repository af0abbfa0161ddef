"""YOLOv3-tiny without a GPU: the max-pool rule, the graph (maxpool nodes, refusals, two heads, channel padding), the padded weights
and the Darknet tiny file.  The device tests are in tests/test_tiny_gpu.py; the recipes in tests/tiny_cases.py."""
import os
import struct

import numpy as np
import pytest

from tests import tiny_cases as TC
from yolo_v3_tf2_amd.graph import AuxOp, ConvOp, _Builder, build_program, load_program
from yolo_v3_tf2_amd.maxpool import maxpool2x2_ref


# ---------------------------------------------------------------------------------------------- the pool rule
@pytest.mark.parametrize("kind", ["normal", "negative", "inf"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", TC.POOL_EXTENTS)
def test_maxpool_ref_equals_the_loop_and_torch(hw, stride, kind):
    """maxpool2x2_ref == the brute-force loop == torch.nn.functional.max_pool2d on the CPU over the input padded with -inf below and to
    the right (Keras 'same' for a 2x2 window: all the padding goes behind; it never wins)."""
    torch = pytest.importorskip("torch")
    h, w = hw
    if stride == 2 and (h % 2 or w % 2):
        with pytest.raises(ValueError, match="even extents"):
            maxpool2x2_ref(np.zeros((1, h, w, 4), np.float32), 2)
        return
    x = TC.pool_data((2, h, w, 8), kind)
    got = maxpool2x2_ref(x, stride)
    assert got.dtype == np.float32 and got.shape == (2, h // stride, w // stride, 8)
    assert np.array_equal(got, TC.maxpool_loop(x, stride))
    t = torch.from_numpy(x).permute(0, 3, 1, 2)
    if stride == 1:
        t = torch.nn.functional.pad(t, (0, 1, 0, 1), value=float("-inf"))
    ref = torch.nn.functional.max_pool2d(t, 2, stride).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(got, ref)
    if kind == "negative":
        assert (got < 0).all()
    if kind == "inf":
        assert np.isneginf(got).any() and np.isposinf(got).any()


def test_maxpool_ref_refuses_bad_arguments():
    with pytest.raises(ValueError):
        maxpool2x2_ref(np.zeros((2, 2, 4), np.float32), 1)
    with pytest.raises(ValueError):
        maxpool2x2_ref(np.zeros((1, 2, 2, 4), np.float32), 3)


# ---------------------------------------------------------------------------------------------- the graph
def test_generated_tiny_yaml_lowers_to_the_tiny_program():
    p = TC.tiny_program(80)
    convs = p.conv_ops()
    aux = [o.kind for o in p.ops if isinstance(o, AuxOp)]
    assert len(convs) == 13 and len(p.conv_nodes) == 13
    assert aux.count("maxpool_s2") == 5 and aux.count("maxpool_s1") == 1 and aux.count("upsample") == 1 and aux.count("concat") == 1
    assert len(aux) == 8 and len(p.ops) == 21
    assert [n.filters for n in p.conv_nodes] == [16, 32, 64, 128, 256, 512, 1024, 256, 512, 255, 128, 256, 255]
    assert len(p.outputs) == 2 and [p.tensors[o].div for o in p.outputs] == [32, 16]
    assert p.grid_sizes(416) == [13, 26] and sum(3 * g * g for g in p.grid_sizes(416)) == 2535
    assert p.grid_sizes((96, 64)) == [(3, 2), (6, 4)]
    # conv0's 16 channels are stored as 32, through pool 0, and conv1 reads 32; nothing else is padded
    c0, c1 = convs[0], convs[1]
    assert (c0.cin, c0.cout) == (3, 32) and (c1.cin, c1.cout, c1.c0) == (32, 32, 32)
    padded = {t: c for t, (c, d) in enumerate(zip(p.stored, p.tensors)) if c != d.channels}
    assert padded == {c0.dst: 32, c1.src0: 32} and c0.dst != c1.src0
    # the real widths stay where they were: the nodes, the tensors, the FLOP count, the weight shapes
    assert p.tensors[c0.dst].channels == 16 and p.conv_nodes[0].filters == 16
    assert p.flops_per_image(416) == sum(2.0 * n.size ** 2 * p.tensors[n.inputs[0]].channels * n.filters * (416 // p.tensors[n.output].div) ** 2
                                         for n in p.conv_nodes)
    # the concat [up(128), 256] feeds a 3x3 conv: the aux kernels carry it, nothing is folded
    cat = [o for o in p.ops if isinstance(o, AuxOp) and o.kind == "concat"][0]
    assert [p.tensors[t].channels for t in cat.inputs] == [128, 256]
    assert all(o.src1 < 0 and not o.src0_upsample and o.residual < 0 for o in convs)
    # YOLOv3 itself: nothing is padded
    p3 = load_program(os.path.join(TC.ROOT, "config", "models", "yolov3", "model.yaml"), 80)
    assert p3.stored == [t.channels for t in p3.tensors] and len(p3.outputs) == 3


def test_reference_tiny_yaml_lowers_to_the_same_program():
    if not os.path.exists(TC.REFERENCE_TINY_MODEL):
        pytest.skip("no checkout of the reference project here")
    ours, ref = TC.tiny_program(80), load_program(TC.REFERENCE_TINY_MODEL, 80)
    assert len(ours.nodes) == len(ref.nodes)
    for a, b in zip(ours.nodes, ref.nodes):
        assert a == b
    assert ours.tensors == ref.tensors and ours.ops == ref.ops and ours.outputs == ref.outputs and ours.stored == ref.stored


def _pool(size=(2, 2), stride=(2, 2), padding="same", **extra):
    conf = {"type": "maxpool", "size_xy": list(size), "stride_xy": list(stride)}
    if padding is not None:
        conf["padding"] = padding
    conf.update(extra)
    return conf


@pytest.mark.parametrize("conf,word", [
    (_pool(size=(3, 3)), "size 3"),
    (_pool(size=(2, 2), stride=(3, 3)), "stride 3"),
    (_pool(padding="valid"), "'valid'"),
    (_pool(padding=None), "'valid'"),
    (_pool(size=(2, 3)), "equal x and y"),
    (_pool(stride=(2, 1)), "equal x and y"),
    (_pool(size=(2,)), "equal x and y"),
    ({"type": "maxpool", "size": 2, "stride": 2, "padding": "same"}, "size_xy"),
])
def test_every_other_pool_is_refused_by_name(conf, word):
    b = _Builder(0, None)
    x = b.new_tensor(32, 1, "input")
    with pytest.raises(ValueError, match="maxpool") as e:
        b.sub_model_layers([conf], x, "backbone")
    assert word in str(e.value) and "backbone.maxpool" in str(e.value)


def test_a_stride_2_pool_at_div_32_is_refused_and_a_stride_1_pool_is_not():
    b = _Builder(0, None)
    x = b.new_tensor(32, 1, "input")
    layers = b.sub_model_layers([_pool()] * 5, x, "backbone")
    assert [b.tensors[t].div for t in layers] == [2, 4, 8, 16, 32]
    assert [n.kind for n in b.nodes] == ["maxpool"] * 5 and all(n.stride == 2 and n.size == 2 for n in b.nodes)
    with pytest.raises(ValueError, match=r"backbone\.maxpool.*1/32"):
        b.maxpool(layers[-1], _pool(), "backbone")
    t = b.maxpool(layers[-1], _pool(stride=(1, 1)), "backbone")
    assert b.tensors[t].div == 32 and b.nodes[-1].stride == 1


def test_a_route_with_three_sources_stays_refused():
    b = _Builder(0, None)
    x = b.new_tensor(32, 1, "input")
    with pytest.raises(ValueError, match="Invalid number of layers: 3"):
        b.sub_model_layers([_pool(stride=(1, 1)), _pool(stride=(1, 1)), _pool(stride=(1, 1)),
                            {"type": "route", "source": {"layers": [0, 1, 2]}}], x, "neck")


def test_padding_rule_pads_only_conv_to_conv_chains():
    """A narrow conv output is padded when convs read it directly or through pools only; an output, or a tensor an add / concat /
    up-sample reads, keeps its width."""
    from tests.helpers import _Graph
    g = _Graph(3)
    a = g.conv(g.input, 16, 3)                 # -> conv directly: padded
    b_ = g.conv(a, 48, 3)                      # -> pool -> pool -> two convs: padded with its pools
    p1 = g._keep(g.b.maxpool(b_, _pool(), "body"))
    p2 = g._keep(g.b.maxpool(p1, _pool(stride=(1, 1)), "body"))
    c = g.conv(p2, 64, 1)
    d = g.conv(p2, 40, 1)                      # an output: not padded
    e = g.conv(c, 24, 1)                       # read by an up-sample: not padded
    u = g.upsample(e)
    p = g.program([d, c, u])
    want = {a: 32, b_: 64, p1: 64, p2: 64}
    assert {t: s for t, (s, d_) in enumerate(zip(p.stored, p.tensors)) if s != d_.channels} == want
    by_dst = {o.dst: o for o in p.conv_ops()}
    assert (by_dst[b_].cin, by_dst[b_].cout) == (32, 64) and (by_dst[c].cin, by_dst[d].cin, by_dst[d].cout) == (64, 64, 40)


# ---------------------------------------------------------------------------------------------- padded weights
def test_padded_weights_hold_zeros_where_stated_and_change_no_real_channel():
    from yolo_v3_tf2_amd.weights import pad_weights
    p = TC.tiny_program(3)
    w, x = TC.tiny_inputs(p, 2, (64, 96))
    pw = pad_weights(p, w)
    assert set(pw) == set(w)
    assert pw["conv0.w"].shape == (3, 3, 3, 32) and pw["conv1.w"].shape == (3, 3, 32, 32)
    assert np.array_equal(pw["conv0.w"][..., :16], w["conv0.w"]) and not pw["conv0.w"][..., 16:].any()
    assert np.array_equal(pw["conv1.w"][:, :, :16], w["conv1.w"]) and not pw["conv1.w"][:, :, 16:].any()
    for k, fill in (("gamma", 0.0), ("beta", 0.0), ("mean", 0.0), ("var", 1.0)):
        assert np.array_equal(pw[f"conv0.{k}"][:16], w[f"conv0.{k}"]) and (pw[f"conv0.{k}"][16:] == fill).all()
        assert np.array_equal(pw[f"conv1.{k}"], w[f"conv1.{k}"])            # conv1's output is not padded
    for i in range(2, 13):
        assert all(pw[k] is w[k] for k in w if k.startswith(f"conv{i}."))
    real, padded = TC.walk(p, w, x), TC.walk(p, w, x, padded=True)
    assert set(real) == set(padded)
    for t, v in real.items():
        c = p.tensors[t].channels
        if v.ndim == 4:
            assert padded[t].shape[-1] == p.stored[t]
            assert np.array_equal(padded[t][..., :c], v), t
            assert not padded[t][..., c:].any(), t          # exact zeros, through BN, leaky and the pool
        else:
            assert np.array_equal(padded[t], v), t
    assert padded[p.conv_ops()[0].dst].shape[-1] == 32


# ---------------------------------------------------------------------------------------------- Darknet tiny file
def test_darknet_tiny_file_round_trip(tmp_path):
    from yolo_v3_tf2_amd.weights import read_darknet_weights, write_darknet_weights
    p = TC.tiny_program(80)
    w, _ = TC.tiny_inputs(p, 1, (32, 32))
    path = str(tmp_path / "yolov3-tiny.weights")
    write_darknet_weights(path, p, w)
    # the published file's size: 5 header words + 8,858,734 floats
    assert os.path.getsize(path) == 4 * (5 + p.n_params()) and p.n_params() == 8858734
    back = read_darknet_weights(path, p)
    assert set(back) == set(w)
    for k in w:
        assert back[k].shape == w[k].shape and np.array_equal(back[k], w[k]), k
    assert back["conv0.w"].shape == (3, 3, 3, 16) and back["conv1.w"].shape == (3, 3, 16, 32)      # real widths in the file
    with open(path, "ab") as f:
        f.write(b"\0")
    with pytest.raises(ValueError, match="trailing bytes"):
        read_darknet_weights(path, p)


def test_darknet_tiny_file_laid_out_by_hand(tmp_path):
    """The file order is the conv order as lowered, per conv [beta, gamma, mean, var] x Cout (a bias conv: bias) then the weights
    (Cout, Cin, kh, kw): written here with struct.pack from a counter and read back element by element."""
    from yolo_v3_tf2_amd.weights import read_darknet_weights
    p = TC.tiny_program(2)
    path = str(tmp_path / "by_hand.weights")
    start, at = {}, 0
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", 0, 2, 5, 0, 0))
        for n in p.conv_nodes:
            cin, cout, k = p.tensors[n.inputs[0]].channels, n.filters, n.size
            count = (4 * cout if n.bn else cout) + cout * cin * k * k
            start[n.conv_index] = at
            f.write(struct.pack(f"<{count}f", *[float(v % 4093) for v in range(at, at + count)]))      # exact in fp32, position-coded
            at += count
    w = read_darknet_weights(path, p)
    assert [n.conv_index for n in p.conv_nodes] == list(range(13))
    for n in p.conv_nodes:
        i, cin, cout, k, s = n.conv_index, p.tensors[n.inputs[0]].channels, n.filters, n.size, start[n.conv_index]
        val = lambda pos: np.float32(pos % 4093)
        if n.bn:
            for j, key in enumerate(("beta", "gamma", "mean", "var")):
                for c in (0, cout // 2, cout - 1):
                    assert w[f"conv{i}.{key}"][c] == val(s + j * cout + c), (i, key, c)
            s += 4 * cout
        else:
            for c in (0, cout - 1):
                assert w[f"conv{i}.bias"][c] == val(s + c)
            s += cout
        hwio = w[f"conv{i}.w"]
        assert hwio.shape == (k, k, cin, cout)
        for (o, ci, u, v) in ((0, 0, 0, 0), (cout - 1, cin - 1, k - 1, k - 1), (cout // 2, cin // 3, k // 2, 0)):
            assert hwio[u, v, ci, o] == val(s + ((o * cin + ci) * k + u) * k + v), (i, o, ci, u, v)


# ---------------------------------------------------------------------------------------------- data files and the binding
def test_tiny_anchor_file_holds_the_published_anchors_coarsest_first():
    a = TC.tiny_anchors()
    assert a.shape == (2, 3, 2)
    px = np.array([[(81, 82), (135, 169), (344, 319)], [(10, 14), (23, 27), (37, 58)]], np.float32)
    assert np.abs(a * 416 - px).max() < 1e-4


def test_generated_files_are_what_the_generator_writes(tmp_path):
    import subprocess
    import sys
    out = tmp_path / "m"
    subprocess.check_call([sys.executable, os.path.join(TC.ROOT, "tools", "gen_model_config.py"), "--model", "tiny", "--out", str(out),
                           "--data", str(tmp_path / "d")], cwd=str(tmp_path))
    for name in ("backbone", "neck0", "head0", "neck1", "head1"):
        assert (out / f"{name}.yaml").read_text() == open(os.path.join(os.path.dirname(TC.TINY_MODEL), f"{name}.yaml")).read(), name
    assert (tmp_path / "d" / "anchors_tiny.txt").read_text() == open(TC.TINY_ANCHORS).read()


def test_new_entries_are_bound_and_refuse_bad_arguments_without_a_device():
    import ctypes as C
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    for name in ("y3_net_create_heads", "y3_net_heads", "y3_maxpool2x2", "y3_yolo_decode_hw_n", "y3_yolo_decode_scores_hw_n",
                 "y3_yolo_decode_candidates_hw_n", "y3_decode_candidates_workspace_bytes_n"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert (_lib.Y3_AUX_MAXPOOL2X2_S2, _lib.Y3_AUX_MAXPOOL2X2_S1) == (3, 4)
    assert lib.y3_net_heads(None) == 0
    fake = C.c_void_p(4096)
    INV = _lib.Y3_ERR_INVALID
    for args, word in (((None, fake, 1, 2, 2, 32, 2, 0), b"bad argument"), ((fake, fake, 1, 2, 2, 32, 3, 0), b"stride"),
                       ((fake, fake, 1, 3, 2, 32, 2, 0), b"even extents"), ((fake, fake, 1, 2, 2, 32, 2, 2), b"dtype"),
                       ((fake, fake, 1, 2, 2, 6, 1, 0), b"16 bytes"), ((fake, C.c_void_p(4100), 1, 2, 2, 32, 1, 1), b"aligned")):
        assert lib.y3_maxpool2x2(*args, None) == INV
        assert b"y3_maxpool2x2" in lib.y3_last_error() and word in lib.y3_last_error(), (args, lib.y3_last_error())
    # the workspace query follows the scale count: tiny at 416 has 2535 boxes, YOLOv3 10647
    gs = (C.c_int32 * 6)(13, 13, 26, 26, 52, 52)
    assert lib.y3_decode_candidates_workspace_bytes_n(gs, 2, 64, 80) == 64 * 2535 * 4
    assert lib.y3_decode_candidates_workspace_bytes_n(gs, 3, 64, 80) == lib.y3_decode_candidates_workspace_bytes(gs, 64, 80) == 64 * 10647 * 4
    assert lib.y3_decode_candidates_workspace_bytes_n(gs, 0, 64, 80) == 0 and lib.y3_decode_candidates_workspace_bytes_n(gs, 4, 64, 80) == 0
    ptrs = (C.c_void_p * 3)(4096, 4096, 4096)
    a = (C.c_float * 18)()
    for n in (0, 4):
        assert lib.y3_yolo_decode_hw_n(ptrs, gs, n, 1, 80, a, fake, fake, fake, None) == INV and b"scales" in lib.y3_last_error()
        assert lib.y3_yolo_decode_scores_hw_n(ptrs, gs, n, 1, 80, a, fake, fake, fake, None) == INV
    # y3_net_create_heads: 2 or 3 outputs
    t = (_lib.TensorDesc * 2)(_lib.TensorDesc(3, 1), _lib.TensorDesc(32, 1))
    k = (C.c_int32 * 1)(0)
    c = (_lib.ConvDesc * 1)(_lib.ConvDesc(3, 1, 3, 32, 1, 1, 0, 0, 3, -1, -1, 1, 1, 1))
    x = (_lib.AuxDesc * 1)()
    h = C.c_void_p()
    for n in (1, 4):
        assert lib.y3_net_create_heads(t, 2, k, 1, c, 1, x, 0, 0, (C.c_int32 * 4)(1, 1, 1, 1), n, 0, C.byref(h)) == INV
        assert b"2 or 3 outputs" in lib.y3_last_error() and not h.value


def test_drop_in_layer_reads_the_tiny_config():
    """core/parse_model.py builds the two-head model from the tiny model.yaml, and the host decode takes the six-row anchors file."""
    import yaml
    from yolo_v3_tf2_amd.core.parse_model import ParseModel
    from yolo_v3_tf2_amd.core.yolo_decode_layer import yolo_decode_hw_host
    cfg = yaml.safe_load(open(os.path.join(TC.ROOT, "config", "detect_config_tiny.yaml")))
    assert cfg["model_config_file"] == "config/models/yolov3_tiny/model.yaml" and cfg["anchors_file"] == "datasets/coco2012/anchors_tiny.txt"
    cwd = os.getcwd()
    os.chdir(TC.ROOT)
    try:
        m = ParseModel().create_model(80, cfg["model_config_file"])
    finally:
        os.chdir(cwd)
    assert len(m.program.outputs) == 2 and len(m.program.conv_ops()) == 13
    rng = np.random.default_rng(5)
    grids = [rng.standard_normal((2, g, g, 3, 12)).astype(np.float32) for g in (3, 6)]
    b, c, pr = yolo_decode_hw_host(grids, TC.tiny_anchors(), 7)
    assert b.shape == (2, 135, 4) and c.shape == (2, 135, 1) and pr.shape == (2, 135, 7)
    from oracle import oracle as O
    ob, oc, op = O.yolo_decode(grids, TC.tiny_anchors(), 7)
    assert np.abs(b - ob).max() <= 1e-5 * max(1.0, np.abs(ob).max()) and np.abs(c - oc).max() <= 1e-6 and np.abs(pr - op).max() <= 1e-6
