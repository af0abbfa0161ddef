"""The layer cases of the split-K suites (tests/test_splitk_gpu.py, tests/test_splitk_bf16_gpu.py, tests/test_splitk_f16_gpu.py), in a module
that needs neither torch nor a GPU so that host tiers (tests/bn_stat_cases.py) can build the same programs."""

C3 = dict(size=3)
# fp32 plans: name -> (in_ch, image size, B, chain, heads, slots that are split); the conv under test is three times the same head, or a chain conv
LAYERS_F32 = {
    # M = 169: ragged last tile; K = 576: 18 K tiles -- S = 2, 3 divide evenly, 4 -> slices of 4, 5, 4, 5 tiles, 8 -> two and three
    "c64_13": (64, 13, 1, [], [dict(filters=64, **C3)] * 3, (0, 1, 2)),
    # the same conv with leaky and a shortcut from the input: residual and activation of the finish kernel
    "c64_13_res": (64, 13, 1, [dict(filters=64, size=1), dict(filters=64, size=3, shortcut=-3)], [dict(filters=64, size=1)] * 3, (1,)),
    # Cin = 256: the default chunk-major K order (128 channels per chunk, 36 K tiles per chunk, 4 per tap) is in force
    "c256_13": (256, 13, 1, [], [dict(filters=128, **C3)] * 3, (0, 1, 2)),
    # stride 2 at 14 x 14: padding taps in every slice
    "s2_14": (64, 14, 1, [], [dict(filters=128, size=3, stride=2)] * 3, (0, 1, 2)),
    # the head shape: 255 channels (CoutPad 256), bias, linear -- the scalar form of the finish kernel; 4 K tiles
    "head255": (128, 13, 1, [], [dict(filters=255, size=1, bn=False, act="linear")] * 3, (0, 1, 2)),
    # three images at 14 x 14: M = 588 spans ten tiles and the image boundaries
    "b3_14": (64, 14, 3, [], [dict(filters=128, **C3)] * 3, (0, 1, 2)),
}

# bf16 / fp16 plans.
H1 = [dict(filters=64, size=1)] * 3
# name -> (in_ch, image size, B, chain, heads, slots that are split).  Every split conv reads the net's input (and takes its shortcut from
# it), so the oracle's reference is teacher-forced; a split chain conv stores bf16, a split head conv writes the fp32 output itself.
LAYERS_16 = {
    # M = 169: ragged last tile; K = 1152: 18 K tiles of 64, two per tap -- S = 2, 3 divide evenly, 4 -> slices of 4, 5, 4, 5 tiles,
    # 8 -> twos and threes with slice starts inside a tap
    "c128_13": (128, 13, 1, [dict(filters=128, **C3)], H1, (0,)),
    # Cout = 64: CoutPad 64, one N tile, only tile 11 fits (the n64 candidates of choose_tile_bf16)
    "c64_13": (128, 13, 1, [dict(filters=64, **C3)], H1, (0,)),
    "c64_13_head": (128, 13, 1, [], [dict(filters=64, **C3)] * 3, (0, 1, 2)),
    # Cin = 64, 3x3 / stride 1, writing an fp32 output itself: not a weight-resident (tile 32) conv, so it splits; 9 K tiles
    "cin64_13_head": (64, 13, 1, [], [dict(filters=64, **C3)] * 3, (0, 1, 2)),
    "c128_13_head": (128, 13, 1, [], [dict(filters=128, **C3)] * 3, (0, 1, 2)),
    # the same conv with leaky and a shortcut from the input: residual and activation of the finish kernel, bf16 output
    "c128_13_res": (128, 13, 1, [dict(filters=128, size=3, shortcut=-2)], H1, (0,)),
    # stride 2 at 14 x 14: padding taps in every slice
    "s2_14": (128, 14, 1, [dict(filters=128, size=3, stride=2)], H1, (0,)),
    "s2_14_head": (128, 14, 1, [], [dict(filters=128, size=3, stride=2)] * 3, (0, 1, 2)),
    # the head shape: 255 channels (CoutPad 256), bias, linear, fp32 output -- 4 K tiles
    "head255": (256, 13, 1, [], [dict(filters=255, size=1, bn=False, act="linear")] * 3, (0, 1, 2)),
    # three images at 14 x 14: M = 588 spans ten tiles and the image boundaries
    "b3_14": (128, 14, 3, [dict(filters=128, **C3)], [dict(filters=128, **C3)] * 3, (0,)),
    "b3_14_head": (128, 14, 3, [], [dict(filters=128, **C3)] * 3, (0, 1, 2)),
}
