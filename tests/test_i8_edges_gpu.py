"""int8 plans on the data the random-input suites never produce (tests/i8_edge_cases.py; what each case is for is asserted on the host
by tests/test_i8_edges_host.py): rounding ties, saturation on both sides of the clamp, accumulators beyond 2^24, the edge channels of
the weight quantiser and the BN fold, the calls in another order, and the real network under scales a quarter of its calibration's.
Every comparison is against yolo_v3_tf2_amd/quant.py with np.array_equal: no tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import i8_edge_cases as E  # noqa: E402
from tests.test_i8_gpu import _check_convs, _cuda  # noqa: E402
from yolo_v3_tf2_amd import _lib, quant  # noqa: E402

I8 = _lib.Y3_DTYPE_I8


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _force_tile(net, tile):
    """Force `tile` on every conv it divides; -> how many."""
    bn = _lib.TILES_BF16[tile][1]
    forced = 0
    for slot, o in enumerate(net.conv_ops):
        if ((o.cout + 31) // 32 * 32) % bn == 0:
            net.set_tile_bf16(slot, tile)
            forced += 1
    return forced


def _forward_and_check(net, p, w, scales, x):
    """One forward; the input's int8 copy against quant.quantize, every conv teacher-forced from the device's own bytes."""
    B = x.shape[0]
    grids = net.forward(_cuda(x).to(torch.float16))
    torch.cuda.synchronize()
    assert net.i8_first_conv() == 0
    assert np.array_equal(net.read_tensor_i8(p.input_tensor, B).cpu().numpy(), quant.quantize(x, scales[p.input_tensor]))
    assert _check_convs(net, p, w, scales, B, grids, 0) == len(p.conv_ops())
    return grids


@pytest.mark.parametrize("tile", E.TILES)
@pytest.mark.parametrize("name", list(E.BUILDERS))
def test_i8_edge_case_bit_exact(rt, name, tile):
    case, xq, ref = E.get(name)
    p = case.program
    assert _lib.tile_built(I8, tile)
    net = rt.Net(p)
    net.load_weights(case.weights)
    net.set_act_scales(case.scales)
    assert _force_tile(net, tile) == len(net.conv_ops)      # every conv of these programs is 128, 255 or 256 wide
    net.keep_activations(True)
    net.plan(case.B, case.canvas, I8)
    grids = _forward_and_check(net, p, case.weights, case.scales, case.x)
    # every conv equal from equal inputs and the input equal: the free-running reference, the one the host test's shares were taken on
    for t in case.stored.values():
        assert np.array_equal(net.read_tensor_i8(t, case.B).cpu().numpy(), ref[t]), t
    for t, g in zip(p.outputs, grids):
        assert np.array_equal(g.cpu().numpy().reshape(ref[t].shape), ref[t]), t


def test_i8_replan_with_new_scales_then_weights_into_the_planned_net(rt):
    """One net, one program: plan with scales A; new scales and plan again; new weights into the planned net, no plan after them
    (the second caller of upload_i8_scales).  Each state bit-exact against the restatement of that state."""
    case, scales_b, second = E.call_order_case()
    p = case.program
    net = rt.Net(p)
    net.load_weights(case.weights)
    net.set_act_scales(case.scales)
    net.keep_activations(True)
    net.plan(case.B, case.canvas, I8)
    _forward_and_check(net, p, case.weights, case.scales, case.x)
    net.set_act_scales(scales_b)
    net.plan(case.B, case.canvas, I8)
    assert net.act_scales() == scales_b
    _forward_and_check(net, p, case.weights, scales_b, case.x)
    net.load_weights(second)
    _forward_and_check(net, p, second, scales_b, case.x)


# ---------------------------------------------------------------------------------------------- the deployed case
@pytest.fixture(scope="module")
def tight96(rt, program, weights):
    """The real network at 2 x 96^2 under a quarter of the scales its own calibration gives: what a net sees when the images it meets
    are brighter than its calibration set.  A uniform factor keeps the two sources of the concat convs equal."""
    S, B = 96, 2
    x = np.random.default_rng(1234).random((B, S, S, 3), dtype=np.float32)
    cal = rt.Net(program)
    cal.load_weights(weights)
    scales = [float(np.float32(s) * np.float32(0.25)) for s in cal.calibrate_i8(_cuda(x))]
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_act_scales(scales)
    net.keep_activations(True)
    net.plan(B, S, I8)
    grids = [g.clone() for g in net.forward(_cuda(x))]
    torch.cuda.synchronize()
    return dict(B=B, scales=scales, net=net, grids=grids)


def test_i8_real_network_under_tight_scales_teacher_forced(program, weights, tight96):
    net, B, scales = tight96["net"], tight96["B"], tight96["scales"]
    cut = net.i8_first_conv()
    convs = program.conv_ops()
    assert cut == 9 == quant.first_i8_conv(program)
    t8 = convs[cut - 1].dst      # the boundary copy saturates as well
    q8 = net.read_tensor_i8(t8, B).cpu().numpy()
    assert np.array_equal(q8, quant.quantize(net.read_tensor(t8, B).cpu().numpy(), scales[t8]))
    shares = {t8: float((np.abs(q8.astype(np.int32)) == 127).mean())}
    for o in convs[cut:]:
        if not quant.writes_f32(program, o):
            shares[o.dst] = float((np.abs(net.read_tensor_i8(o.dst, B).cpu().numpy().astype(np.int32)) == 127).mean())
    print("bytes at +-127 per stored tensor:", " ".join(f"{t}:{s:.1%}" for t, s in shares.items()))
    assert max(s for t, s in shares.items() if t != t8) >= 0.05
    assert _check_convs(net, program, weights, scales, B, tight96["grids"], cut) == len(convs) - cut


def test_i8_real_network_under_tight_scales_free_running(program, weights, tight96):
    net, B, scales = tight96["net"], tight96["B"], tight96["scales"]
    cut = net.i8_first_conv()
    t8 = program.conv_ops()[cut - 1].dst
    out = quant.forward_i8(program, weights, scales, {t8: net.read_tensor_i8(t8, B).cpu().numpy()}, cut)
    for t, g in zip(program.outputs, tight96["grids"]):
        g = g.cpu().numpy().reshape(out[t].shape)
        assert np.array_equal(g, out[t]) and np.isfinite(g).all() and np.abs(g).max() > 0, t
