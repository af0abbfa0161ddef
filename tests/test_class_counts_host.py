"""The network at class counts other than 80, without a GPU: the program builds, its three head convs have 3 * (5 + nc) filters
with bias, synthetic weights cover them, the oracle runs it, the int8 cut stays where it was, and a Darknet weights file written for
that program reads back into it.  tests/test_class_counts_gpu.py runs the same programs on the device."""
import os

import numpy as np
import pytest

from tests import class_count_cases as K

CLASS_COUNTS = (1, 3, 7, 37, 70, 79, 81)


@pytest.mark.parametrize("nc", CLASS_COUNTS)
def test_program_at_class_count(nc, tmp_path):
    from oracle import oracle as O
    from yolo_v3_tf2_amd import quant
    from yolo_v3_tf2_amd import weights as W
    p = K.program(nc)
    assert p.nclasses == nc and len(p.outputs) == 3 and len(p.conv_ops()) == 75
    heads = K.head_ops(p)
    assert [o.conv_index for o in heads] == [58, 66, 74]
    for o in heads:
        assert o.cout == 3 * (5 + nc) and not o.bn and not o.leaky and o.size == 1 and o.stride == 1
        assert o.src1 < 0 and o.residual < 0 and quant.writes_f32(p, o)
    assert [o.cin for o in heads] == [1024, 512, 256]
    assert K.head_route(nc) == ("fused" if 70 <= nc <= 80 else "composed")
    w = K.weights(nc)
    assert sum(v.size for v in w.values()) == p.n_params()
    for o in heads:
        i = o.conv_index
        assert w[f"conv{i}.w"].shape == (1, 1, o.cin, o.cout) and w[f"conv{i}.bias"].shape == (o.cout,) and f"conv{i}.gamma" not in w
        assert np.isfinite(w[f"conv{i}.w"]).all() and float(w[f"conv{i}.w"].std()) > 0
    assert quant.first_i8_conv(p) == 9
    # the oracle forward at 2 x 64^2: shapes, and logits that are neither constant nor saturated
    x, ref = K.oracle_grids(nc)
    assert x.shape == (2, 64, 64, 3)
    for g, s in zip(ref, (2, 4, 8)):
        assert g.shape == (2, s, s, 3, 5 + nc) and g.dtype == np.float32 and np.isfinite(g).all()
        assert 1e-3 < float(g.std()) and float(np.abs(g).max()) < 50.0
        assert all(float(g[..., k].std()) > 1e-4 for k in range(5 + nc)), "a head channel is constant"
    # Darknet round trip (what tests/test_weights.py::test_darknet_layout_round_trip uses)
    path = str(tmp_path / f"nc{nc}.weights")
    W.write_darknet_weights(path, p, w)
    assert os.path.getsize(path) == 20 + 4 * p.n_params()
    back = W.read_darknet_weights(path, p)
    assert sorted(back) == sorted(w) and all(np.array_equal(back[k], w[k]) for k in w)
    if nc != 80:      # and the file does not fit the 80-class program: the head convs differ in size
        with pytest.raises(ValueError):
            W.read_darknet_weights(path, K.program(80))
    os.remove(path)      # a quarter of a gigabyte per class count


def test_head_widths_and_paddings():
    """The widths the issue of this suite names: 18 / 24 / 36 / 126 even and ragged, 225 and 252 inside the 256-wide fused tile,
    258 past it."""
    assert [3 * (5 + nc) for nc in (1, 3, 7, 37, 70, 79, 81)] == [18, 24, 36, 126, 225, 252, 258]
    assert [K.head_route(nc) for nc in (1, 69, 70, 80, 81)] == ["composed", "composed", "fused", "fused", "composed"]
