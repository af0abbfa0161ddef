"""The four y3_net_set_tile* entry points accept exactly the (conv, tile id) pairs a restatement from the Python-side tile tables
and the conv descriptors says they should.  Needs a device only because y3_net_create does; nothing is planned or launched."""
import pytest

pytestmark = pytest.mark.gpu


def _output_staged(ops, t):
    """csrc/y3_net.cpp output_staged: a conv reads net output t again, or a shortcut / first-layer conv writes it."""
    return any(t in (o.src0, o.src1, o.residual) or (o.dst == t and (o.residual >= 0 or o.cin == 3)) for o in ops)


def _accepts(_lib, mode, program, ops, o, tile):
    table = {"f32": _lib.TILES, "bf16": _lib.TILES_BF16, "f32x3": _lib.TILES_X3, "f32x2": _lib.TILES_X3}[mode]
    if tile == -1:
        return True                      # back to the table / the heuristic
    if tile < 0 or tile >= len(table):
        return False
    built = {"f32": table[tile][0] > 0, "bf16": table[tile][0] > 0, "f32x3": tile in _lib.TILES_X3_BUILT,
             "f32x2": tile in _lib.TILES_X2_BUILT}[mode]
    if not built or o.cin == 3:          # retired id / the first layer has its own kernel
        return False
    bn, last = table[tile][1], table[tile][3]
    cout_pad = (o.cout + 31) // 32 * 32 if mode in ("f32", "bf16") else (o.cout + 63) // 64 * 64
    if cout_pad % bn:
        return False
    if mode != "f32" and (o.cin % last or (o.src1 >= 0 and o.c0 % last)):      # last = BK in these three tables
        return False
    res_shape = o.size == 3 and o.stride == 1 and o.src1 < 0 and o.cout % 64 == 0
    if mode == "f32" and tile == 33:
        return res_shape and o.cin == 32
    if mode == "bf16" and tile == 32:    # stores bf16 only: not for a net output handed over as fp32 straight from the launch
        return res_shape and o.cin in (32, 64) and not (o.dst in program.outputs and not _output_staged(ops, o.dst))
    return True


@pytest.mark.parametrize("mode", ["f32", "bf16", "f32x3", "f32x2"])
def test_setters_accept_exactly_the_fitting_built_tiles(program, mode):
    from yolo_v3_tf2_amd import _lib, runtime
    _lib.require_gpu()
    net = runtime.Net(program)           # unplanned, no weights: the setters need neither
    fn = getattr(net.lib, {"f32": "y3_net_set_tile", "bf16": "y3_net_set_tile_bf16", "f32x3": "y3_net_set_tile_x3",
                           "f32x2": "y3_net_set_tile_x2"}[mode])
    count = len({"f32": _lib.TILES, "bf16": _lib.TILES_BF16, "f32x3": _lib.TILES_X3, "f32x2": _lib.TILES_X3}[mode])
    ops = net.conv_ops
    assert len(ops) == 75 and sum(o.src1 >= 0 for o in ops) == 2 and ops[0].cin == 3
    wrong = []
    n_ok = 0
    for slot, o in enumerate(ops):
        for tile in range(-1, count + 2):
            st = fn(net._h, slot, tile)
            assert st in (_lib.Y3_OK, _lib.Y3_ERR_INVALID), (slot, tile, st)
            want = _accepts(_lib, mode, program, ops, o, tile)
            n_ok += want
            if (st == _lib.Y3_OK) != want:
                wrong.append((slot, tile, st))
    assert not wrong, wrong[:20]
    assert n_ok > len(ops)               # the restatement is not vacuous: more than the -1 of every slot is accepted
    assert fn(net._h, -1, 0) == _lib.Y3_ERR_INVALID and fn(net._h, len(ops), 0) == _lib.Y3_ERR_INVALID
    assert fn(None, 0, 0) == _lib.Y3_ERR_INVALID
