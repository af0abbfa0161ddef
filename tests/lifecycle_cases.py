"""What tests/test_lifecycle_host.py and tests/test_lifecycle_gpu.py share: one long-lived Net through many plans against a freshly
planned TWIN, bit for bit.

A Net is planned again whenever the batch shape changes (Net._plan_for), by set_dtype and by calibrate_i8, and keeps a lot of state
across y3_net_plan_hw.  The parity suites compare a net with the oracle on its first plan; here a WALK -- a list of steps on one net --
is replayed on the device, and at every forward / detect / read step a fresh Net is configured with the FOLD of the steps so far, planned
once, and must give the same bits.  No tolerance anywhere: one library on one input (tests/test_gpu_parity.py::
test_forward_is_deterministic; split-K "summed in a fixed order").

Steps (tuples):
  ("plan", max_batch, canvas, mode | None)      Net.plan; mode None: the net's dtype default
  ("set_dtype", mode)                           Net.set_dtype
  ("set", name, *args)                          getattr(net, name)(*args), name a set_* of Net or keep_activations
  ("attr", name, value)                         setattr(net, name, value): nms_per_class, multi_label
  ("load", seed)                                load_weights(synthetic_weights(program, seed))
  ("scales", id | None)                         set_act_scales of the calibration `id` made once on a separate net (None: all unset)
  ("calibrate", B, canvas)                      calibrate_i8 on the long-lived net; its scales are the calibration ("own", step index)
  ("forward", B[, canvas])  ("detect", B)       run and compare with the twin; a canvas other than the planned one goes through _plan_for
  ("read",)                                     read_tensor of every stored tensor of the last forward, compared with the twin's

The fold restates the survival rules from the docstrings (yolo_v3_tf2_amd/net.py, include/y3.h "Setters on a planned net"):
  * every set_* survives plan() -- "A tile forced through these setters acts at once on a planned net and survives plan()";
  * lanes do not: "plan() sets it from the plan's tuning table (1 without one): call it after plan()";
  * set_tiny_stem_fusion, set_early_chunk, keep_activations and set_act_scales wait for the next plan: the twin takes the values the
    last plan found, not the live ones;
  * plan(dtype=None) takes Net.dtype, which plan() and set_dtype() set and calibrate_i8 leaves at fp32 ("The net is left planned in
    fp32 with activations kept");
  * _plan_for only grows max_batch and keeps the form of the last plan: "a net planned with a pair stays a pair plan ... a net planned
    with an int, or never planned, takes a square batch as an int plan"; calibrate_i8 plans with a pair.

NumPy and the package's host code only."""
import functools
import json
import os
from collections import namedtuple

import numpy as np

from yolo_v3_tf2_amd import _lib

MODES = ("f32", "bf16", "f16", "f32x3", "f32x2", "i8")
DTYPE = {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16, "f16": _lib.Y3_DTYPE_F16, "f32x3": _lib.Y3_DTYPE_F32X3,
         "f32x2": _lib.Y3_DTYPE_F32X2, "i8": _lib.Y3_DTYPE_I8}
CANVASES = (32, 64, 96, (64, 96))
MAX_IMAGES = 7
MAX_SIDE = 96
WEIGHT_BUDGET = 1_500_000
IMAGE_SEED = 2024
# synthetic_weights gives the heads an objectness bias of -4 and class biases of -1: conf * prob is about 0.018 * 0.27 = 0.005, so the
# threshold sits below that and every detect step returns rows (the walks require it: equal empty results would say nothing)
MAX_BOXES, IOU, SCORE = 50, 0.5, 0.002
# the one step above MAX_IMAGES: the border skip needs whole blocks of 32 images per lane (include/y3.h, y3_net_set_border_skip), so
# its engagement condition can only be met there -- at 32 x 32 pixels, fewer pixels than four images at 96 x 96
BORDER_BATCH, BORDER_CANVAS = 32, 32


# ---------------------------------------------------------------------------------------------- programs
@functools.lru_cache(maxsize=None)
def program_a(nclasses=5):
    """Darknet-shaped, runs in all six modes.  The first four convs are YOLOv3's (3 -> 32 3x3, 32 -> 64 3x3/2, 64 -> 32 1x1, 32 -> 64
    3x3 + shortcut), then 3x3/2 to 128 and to 256 with a residual block each, a head at 1/8 behind a 3x3 256 -> 128 (K = 2304: the one
    conv the 16-bit split-K rule takes) and a head at 1/4 behind the folding upsample + route.  Every conv from slot 7 (128 -> 256, 3x3/2)
    on has Cin % 128 == 0: the int8 cut falls there and conv 6's output crosses it."""
    from yolo_v3_tf2_amd.graph import Program, _lower
    from tests.helpers import _Graph
    g = _Graph(3)
    c1 = g.conv(g.conv(g.input, 32, 3), 64, 3, stride=2)
    r2 = g.shortcut(g.conv(g.conv(c1, 32, 1), 64, 3, act="linear"), c1)
    c4 = g.conv(r2, 128, 3, stride=2)
    r4 = g.shortcut(g.conv(g.conv(c4, 64, 1), 128, 3, act="linear"), c4)
    c7 = g.conv(r4, 256, 3, stride=2)
    r8 = g.shortcut(g.conv(g.conv(c7, 128, 1), 256, 3, act="linear"), c7)
    nh = 3 * (5 + nclasses)
    h0 = g.conv(g.conv(r8, 128, 3), nh, 1, bn=False, act="linear", sub="head")
    y = g.conv(r8, 128, 1)
    m = g.conv(g.route(g.upsample(y), r4), 128, 1)
    h1 = g.conv(g.conv(m, 128, 3), nh, 1, bn=False, act="linear", sub="head")
    p = Program(g.b.tensors, g.b.nodes, [], g.input, [h0, h1], nclasses)
    p.conv_nodes = [n for n in g.b.nodes if n.kind == "conv"]
    _lower(p)
    return p


@functools.lru_cache(maxsize=None)
def program(key):
    """"a" | "a80" (program A with 5 / 80 classes), "b" (YOLOv3-tiny from its YAML), "c" (tests/helpers.unfolded_program),
    "odd" (tests/odd_width_cases: 96 -> 96 3x3, no 16-bit tile), "noi8" (program C: none of its convs qualifies for int8)."""
    if key in ("a", "a80"):
        return program_a(5 if key == "a" else 80)
    if key == "b":
        from tests.tiny_cases import tiny_program
        return tiny_program(80)
    if key in ("c", "noi8"):
        from tests.helpers import unfolded_program
        return unfolded_program()[0]
    if key == "odd":
        from tests.odd_width_cases import unrunnable_programs
        return unrunnable_programs()["96to96_3x3"][0]
    raise KeyError(key)


PROGRAM_MODES = {"a": MODES, "a80": MODES, "b": ("f32", "bf16", "f16"), "c": ("f32",)}


@functools.lru_cache(maxsize=None)
def weights(key, seed):
    from yolo_v3_tf2_amd.weights import synthetic_weights
    w = synthetic_weights(program(key), seed=seed)
    for v in w.values():
        v.setflags(write=False)
    return w


def out_of_range_weights(key, seed, slot=5):
    """weights(key, seed) with conv `slot`'s BN gamma raised so that a BN-scaled weight reaches 65504: a Y3_DTYPE_F32X2 plan refuses
    them, a forward on such a plan refuses them by name."""
    w = dict(weights(key, seed))
    i = program(key).conv_ops()[slot].conv_index
    big = np.array(w[f"conv{i}.gamma"], np.float32)
    big[0] = 1e9
    w[f"conv{i}.gamma"] = big
    return w


def n_weights(p):
    return sum(n.size * n.size * p.tensors[n.inputs[0]].channels * n.filters for n in p.conv_nodes)


def canvas_hw(canvas):
    return (canvas, canvas) if isinstance(canvas, (int, np.integer)) else tuple(canvas)


@functools.lru_cache(maxsize=None)
def images(key, canvas, batch):
    """fp32 input, read-only; the first images of a larger batch are those of a smaller one."""
    h, w = canvas_hw(canvas)
    cin = program(key).tensors[program(key).input_tensor].channels
    rng = np.random.default_rng(IMAGE_SEED)
    x = np.stack([rng.random((h, w, cin), dtype=np.float32) if cin == 3 else rng.standard_normal((h, w, cin)).astype(np.float32)
                  for _ in range(batch)])
    x.setflags(write=False)
    return x


def anchors(key):
    from tests.tiny_cases import tiny_anchors
    return np.asarray(tiny_anchors(), np.float32)          # six (w, h) pairs: programs A and B have two heads


def stored_tensors(p):
    """Tensors an op writes into the arena: every op's destination that is neither the input nor a head grid."""
    out = []
    for o in p.ops:
        if o.dst not in p.outputs and o.dst != p.input_tensor and o.dst not in out:
            out.append(o.dst)
    return out


def table_lanes(mode, max_batch, image_size):
    """The lanes Net._apply_tuning sets on every plan: the tuning table's, 1 without a table."""
    from yolo_v3_tf2_amd.net import tuning_table_path
    tag = "bf16" if mode in ("f16", "i8") else mode
    path = tuning_table_path(tag, max_batch, image_size)
    if os.path.exists(path) and not os.environ.get("Y3_NO_TUNING"):
        with open(path) as f:
            return int(json.load(f).get("lanes", 1))
    return 1


# ---------------------------------------------------------------------------------------------- the settings fold
# setters whose last call wins and which act at once on a planned net
AT_ONCE = ("set_xcd_mode", "set_k_chunk", "set_border_skip", "set_stem_fusion", "set_stem_fusion_f16", "set_low_latency",
           "set_low_latency_bf16", "set_low_latency_f16", "set_low_latency_i8")
TILE_SETTERS = {"set_tile": "", "set_tile_bf16": "_bf16", "set_tile_x3": "_x3", "set_tile_x2": "_x2"}
SPLIT_SETTERS = {"set_split_k": "", "set_split_k_bf16": "_bf16", "set_split_k_f16": "_f16", "set_split_k_i8": "_i8"}
# setters a planned net does not follow until it is planned again: the twin takes what the last plan found
AT_PLAN = {"set_tiny_stem_fusion": (False,), "set_early_chunk": (0, 0), "keep_activations": (False,)}
ATTRS = {"nms_per_class": False, "multi_label": False}


class State:
    """The effective settings after a prefix of a walk: everything a fresh net needs to be configured with once."""

    def __init__(self):
        self.simple = {}                     # AT_ONCE name -> args
        self.tiles = {}                      # (suffix, slot) -> tile
        self.splits = {}                     # (suffix, slot) -> S
        self.attrs = dict(ATTRS)
        self.pending = dict(AT_PLAN)         # live values of the setters that wait
        self.pending_scales = None
        self.planned = dict(AT_PLAN)         # ... and what the plan in force found
        self.planned_scales = None
        self.dtype = "f32"                   # Net.dtype: what plan(dtype=None) and _plan_for take
        self.max_batch, self.image_size = 0, 0   # image_size in the form of the plan: int or (H, W); 0: no plan
        self.lanes = 1
        self.seed = None
        self.last = None                     # (kind, B) of the last forward / detect on the plan in force

    @property
    def canvas(self):
        return canvas_hw(self.image_size) if self.max_batch else (0, 0)

    def _plan(self, max_batch, image_size, mode):
        self.max_batch, self.dtype = int(max_batch), mode
        self.image_size = int(image_size) if isinstance(image_size, (int, np.integer)) else tuple(image_size)
        self.planned, self.planned_scales = dict(self.pending), self.pending_scales
        self.lanes = table_lanes(mode, self.max_batch, self.image_size)
        self.last = None

    def _plan_for(self, B, canvas):
        h, w = canvas_hw(canvas)
        if (h, w) != self.canvas or B > self.max_batch:
            pair = h != w or isinstance(self.image_size, tuple)
            self._plan(max(B, self.max_batch), (h, w) if pair else h, self.dtype)

    def step(self, s, index=None):
        kind = s[0]
        if kind == "plan":
            self._plan(s[1], s[2], s[3] or self.dtype)
        elif kind == "set_dtype":
            if self.max_batch and s[1] != self.dtype:
                self._plan(self.max_batch, self.image_size, s[1])
            self.dtype = s[1]
        elif kind == "set":
            name, args = s[1], tuple(s[2:])
            if name in AT_ONCE:
                self.simple[name] = args
            elif name in AT_PLAN:
                self.pending[name] = args
            elif name == "set_lanes":
                self.lanes = int(args[0])
            elif name in TILE_SETTERS:
                key = (TILE_SETTERS[name], args[0])
                self.tiles.pop(key, None) if args[1] < 0 else self.tiles.__setitem__(key, args[1])
            elif name in SPLIT_SETTERS:
                key = (SPLIT_SETTERS[name], args[0])
                self.splits.pop(key, None) if args[1] < 0 else self.splits.__setitem__(key, args[1])
            else:
                raise KeyError(name)
        elif kind == "attr":
            self.attrs[s[1]] = s[2]
        elif kind == "load":
            self.seed = s[1]
        elif kind == "scales":
            self.pending_scales = s[1]
        elif kind == "calibrate":
            self.pending["keep_activations"] = (True,)
            h, w = canvas_hw(s[2])
            self._plan(s[1], (h, w), "f32")
            self.last = ("forward", s[1])
            self.pending_scales = ("own", index)
            self.pending["keep_activations"] = (False,)
        elif kind in ("forward", "detect"):
            self._plan_for(s[1], s[2] if len(s) > 2 else (self.image_size if self.max_batch else None))
            self.last = (kind, s[1])
        elif kind != "read":
            raise KeyError(kind)
        return self


def fold(steps):
    st = State()
    for i, s in enumerate(steps):
        st.step(s, i)
    return st


def twin_calls(state):
    """The canonical configuration of the twin: [(when, name, args)] with when "before" or "after" its one plan."""
    calls = [("before", name, state.planned[name]) for name in sorted(AT_PLAN)]
    calls += [("before", name, state.simple[name]) for name in sorted(state.simple)]
    tile_name = {v: k for k, v in TILE_SETTERS.items()}
    calls += [("before", tile_name[sfx], (slot, t)) for (sfx, slot), t in sorted(state.tiles.items())]
    split_name = {v: k for k, v in SPLIT_SETTERS.items()}
    calls += [("before", split_name[sfx], (slot, S)) for (sfx, slot), S in sorted(state.splits.items())]
    calls.append(("after", "set_lanes", (state.lanes,)))
    return calls


# ---------------------------------------------------------------------------------------------- walks
Walk = namedtuple("Walk", "name net steps needs")      # needs: the mechanisms that must be in force at some step (ENGAGEMENTS)
ENGAGEMENTS = ("tiny_stem", "i8_cut", "split_f32", "split_bf16", "split_f16", "split_i8", "border", "lanes", "early")
SPLIT_SLOT = 10        # program A: the 3x3 256 -> 128 in front of head 0


def euler_circuit(nodes=MODES):
    """A closed walk that takes each ordered pair of distinct nodes exactly once (Hierholzer on the complete digraph)."""
    arcs = {a: [b for b in nodes if b != a] for a in nodes}
    stack, out = [nodes[0]], []
    while stack:
        v = stack[-1]
        if arcs[v]:
            stack.append(arcs[v].pop(0))
        else:
            out.append(stack.pop())
    return out[::-1]


def mode_walk():
    """All 30 ordered pairs of the six modes on program A: every arrival is a forward checked against the twin; the transition is
    plan() or set_dtype() in turn, and canvas, batch and lanes change along the way."""
    tour = euler_circuit()
    steps = [("load", 1), ("scales", "shared"), ("plan", 2, 64, tour[0]), ("forward", 2)]
    for k, mode in enumerate(tour[1:]):
        canvas, B, lanes = CANVASES[k % 4], 1 + (3 * k) % MAX_IMAGES, 1 + (k // 2) % 3
        if k % 3 == 1:
            steps.append(("set_dtype", mode))             # same batch and canvas as the plan in force
            steps.append(("forward", fold(steps).max_batch))
        else:
            steps.append(("plan", B, canvas, mode))
            steps.append(("set", "set_lanes", lanes))
            steps.append(("forward", B))
    return Walk("modes", "a", tuple(steps), ("i8_cut", "lanes"))


def _walks():
    out = [mode_walk()]
    out.append(Walk("calibrate_in_the_middle", "a", (
        ("load", 1), ("scales", "shared"), ("plan", 3, 64, "i8"), ("forward", 3), ("calibrate", 2, 32), ("forward", 2), ("read",),
        ("plan", 3, 64, "i8"), ("forward", 3), ("set_dtype", "bf16"), ("forward", 2)), ("i8_cut",)))
    out.append(Walk("growth", "a", (
        ("load", 1), ("forward", 2, 64), ("forward", 5, 64), ("forward", 3, 64), ("forward", 2, (64, 96)), ("forward", 4, 64),
        ("detect", 6, 64), ("forward", 1, 32)), ()))
    for mode in MODES:
        out.append(Walk(f"reload_{mode}", "a", (
            ("scales", "shared"), ("load", 1), ("plan", 3, 64, mode), ("forward", 3), ("load", 2), ("forward", 3), ("forward", 2)),
            ("i8_cut",) if mode == "i8" else ()))
    for mode in PROGRAM_MODES["b"]:
        out.append(Walk(f"reload_tiny_{mode}", "b", (
            ("set", "set_tiny_stem_fusion", True), ("load", 1), ("plan", 2, 64, mode), ("forward", 2), ("load", 2), ("forward", 2)),
            ("tiny_stem",)))
    # switches set in one mode, another mode planned, then back; and switches on the planned net with no new plan
    out.append(Walk("switches_low_latency", "a", (
        ("load", 1), ("scales", "shared"), ("set", "set_low_latency", True), ("set", "set_low_latency_bf16", True),
        ("plan", 1, 64, "bf16"), ("forward", 1), ("set", "set_low_latency_f16", True), ("set", "set_low_latency_i8", True),
        ("plan", 2, 64, "f32"), ("forward", 2), ("set", "set_split_k", SPLIT_SLOT, 3), ("forward", 2),
        ("plan", 1, (64, 96), "f16"), ("forward", 1), ("set", "set_split_k_f16", SPLIT_SLOT, 4), ("forward", 1),
        ("plan", 2, 96, "i8"), ("set", "set_split_k_i8", SPLIT_SLOT, 2), ("set", "set_lanes", 2), ("forward", 2),
        ("plan", 1, 64, "bf16"), ("forward", 1), ("set", "set_low_latency_bf16", False), ("forward", 1),
        ("set", "set_split_k_bf16", SPLIT_SLOT, 4), ("forward", 1), ("set", "set_split_k", SPLIT_SLOT, -1), ("set", "set_low_latency", False), ("plan", 2, 64, "f32"), ("forward", 2)),
        ("split_f32", "split_bf16", "split_f16", "split_i8", "i8_cut", "lanes")))
    # every setter before the net's first plan, then one plan per mode: what a caller configures up front is what every plan finds
    out.append(Walk("setters_before_the_first_plan", "a", (
        ("load", 1), ("scales", "shared"), ("set_dtype", "bf16"), ("set", "set_lanes", 2), ("set", "set_early_chunk", 4, 2), ("set", "keep_activations", True),
        ("set", "set_tile", 4, 11), ("set", "set_tile_bf16", 4, 11), ("set", "set_tile_x3", 7, 1), ("set", "set_tile_x2", 7, 1),
        ("set", "set_split_k", SPLIT_SLOT, 3), ("set", "set_split_k_bf16", SPLIT_SLOT, 4), ("set", "set_split_k_f16", SPLIT_SLOT, 4),
        ("set", "set_split_k_i8", SPLIT_SLOT, 2), ("set", "set_low_latency_f16", True), ("set", "set_low_latency_i8", True),
        ("set", "set_stem_fusion", 2), ("set", "set_stem_fusion_f16", 1), ("set", "set_k_chunk", 32), ("set", "set_xcd_mode", 0),
        ("plan", 3, 64, "f32"), ("forward", 3), ("read",), ("set", "set_early_chunk", 0, 0), ("set", "keep_activations", False),
        ("plan", 2, 64, "bf16"), ("forward", 2), ("scales", None), ("plan", 2, 64, "f16"), ("forward", 2), ("scales", "shared"),
        ("plan", 2, 32, "f32x3"), ("forward", 2),
        ("set_dtype", "f32x2"), ("forward", 2), ("plan", 2, 64, "i8"), ("forward", 2)),
        ("early", "split_f32", "split_bf16", "split_f16", "split_i8", "i8_cut")))
    out.append(Walk("switches_stem_and_tiles", "a", (
        ("load", 1), ("scales", "shared"), ("plan", 3, 64, "f32"), ("forward", 3), ("set", "set_stem_fusion", 0), ("forward", 3),
        ("set", "set_stem_fusion", 2), ("forward", 3), ("set", "set_tile", 4, 11), ("set", "set_k_chunk", 32), ("forward", 3),
        ("plan", 3, 64, "f16"), ("forward", 3), ("set", "set_stem_fusion_f16", 1), ("forward", 3), ("set", "set_tile_bf16", 4, 11),
        ("forward", 2), ("plan", 2, 32, "bf16"), ("forward", 2), ("set", "set_stem_fusion_f16", 2), ("plan", 2, 64, "i8"),
        ("forward", 2), ("set", "set_tile", 4, -1), ("set", "set_k_chunk", 0), ("set", "set_xcd_mode", 0),
        ("plan", 4, (64, 96), "f32"), ("forward", 4), ("set", "set_xcd_mode", 1), ("set", "set_stem_fusion", 1),
        ("set", "set_tile_bf16", 4, -1), ("set", "set_k_chunk", -1), ("forward", 3), ("set", "set_tile_x3", 7, 1),
        ("plan", 2, 64, "f32x3"), ("forward", 2), ("set", "set_tile_x3", 7, -1), ("forward", 2), ("set", "set_tile_x2", 7, 1),
        ("set_dtype", "f32x2"), ("forward", 2), ("set", "set_tile_x2", 7, -1), ("forward", 2)), ("i8_cut",)))
    out.append(Walk("switches_border_and_chunks", "a", (
        ("load", 1), ("set", "set_border_skip", 1), ("plan", BORDER_BATCH, BORDER_CANVAS, "f32"), ("forward", BORDER_BATCH),
        ("set", "set_border_skip", 0), ("forward", BORDER_BATCH), ("set", "set_border_skip", -1), ("set", "set_early_chunk", 4, 2),
        ("forward", 5), ("plan", 5, 64, "f32"), ("set", "set_lanes", 2), ("forward", 5), ("set", "set_early_chunk", 0, 0),
        ("forward", 4), ("plan", 5, 64, "bf16"), ("forward", 5), ("set", "keep_activations", True), ("set", "set_stem_fusion", 0),
        ("set", "set_stem_fusion", 1), ("forward", 3), ("plan", 3, 32, "f32"), ("forward", 3), ("read",)),
        ("border", "early", "lanes")))
    out.append(Walk("switches_detect", "a80", (
        ("load", 1), ("scales", "shared"), ("plan", 3, 64, "f32"), ("detect", 3), ("attr", "nms_per_class", True), ("detect", 3),
        ("attr", "multi_label", True), ("detect", 2), ("plan", 3, 96, "bf16"), ("detect", 3), ("attr", "multi_label", False),
        ("set", "keep_activations", True), ("detect", 3), ("attr", "nms_per_class", False), ("plan", 2, (64, 96), "i8"),
        ("detect", 2), ("read",)), ("i8_cut",)))
    for canvas in (64, (64, 96)):
        tag = "x".join(str(v) for v in canvas_hw(canvas))
        out.append(Walk(f"tiny_stem_{tag}", "b", (
            ("load", 1), ("plan", 2, canvas, "f32"), ("forward", 2), ("set", "set_tiny_stem_fusion", True), ("forward", 2),
            ("plan", 2, canvas, "f32"), ("forward", 2), ("set_dtype", "bf16"), ("forward", 2), ("set", "keep_activations", True),
            ("plan", 3, canvas, "f16"), ("forward", 3), ("set", "set_tiny_stem_fusion", False), ("forward", 1),
            ("set_dtype", "f32"), ("forward", 3), ("read",)), ("tiny_stem",)))
    out.append(Walk("unfolded_add", "c", (
        ("load", 1), ("plan", 2, 32, "f32"), ("forward", 2), ("set", "keep_activations", True), ("forward", 3, (64, 96)), ("read",),
        ("set", "set_lanes", 3), ("forward", 3), ("read",), ("set", "keep_activations", False), ("plan", 4, 64, None), ("forward", 4)),
        ("lanes",)))
    return out


WALKS = _walks()
BY_NAME = {w.name: w for w in WALKS}

# every set_* of Net (tests/test_runtime_surface_host.py, NET_METHODS) must occur in the walks before a plan and on a planned net, or
# be named here with the reason
SETTER_EXEMPT = {
    "set_dtype": "a step kind of its own (\"set_dtype\"), not a setting: it plans",
    "set_act_scales": "a step kind of its own (\"scales\"), before a plan and on a planned net: its argument is the shared calibration",
}
# the setters whose call on a planned net must change the very next forward's bits, in the words of include/y3.h: the fp32 fused stem
# ("conv0's summation order differs between the two kernels") and an fp32 split ("results differ from the default plan's in the last bits")
MUST_DIFFER = ("set_stem_fusion", "set_split_k", "set_low_latency")

# ---------------------------------------------------------------------------------------------- the setters' contract on a planned net
# (name, program, mode, max_batch, canvas, args): after plan + forward, call the setter.  at_once: the next forward equals a twin
# configured that way before its one plan.  waits: the next forward has the bits of the one before; after a new plan it equals the twin.
Contract = namedtuple("Contract", "name net mode max_batch canvas args")
ACTS_AT_ONCE = (
    Contract("set_lanes", "a", "f32", 5, 64, (3,)),
    Contract("set_tile", "a", "f32", 3, 64, (4, 11)),
    Contract("set_tile_bf16", "a", "bf16", 3, 64, (4, 11)),
    Contract("set_tile_x3", "a", "f32x3", 3, 64, (7, 1)),
    Contract("set_tile_x2", "a", "f32x2", 3, 64, (7, 1)),
    Contract("set_low_latency", "a", "f32", 1, 64, (True,)),
    Contract("set_low_latency_bf16", "a", "bf16", 1, 64, (True,)),
    Contract("set_low_latency_f16", "a", "f16", 1, 64, (True,)),
    Contract("set_low_latency_i8", "a", "i8", 1, 64, (True,)),
    Contract("set_split_k", "a", "f32", 2, 64, (SPLIT_SLOT, 4)),
    Contract("set_split_k_bf16", "a", "bf16", 2, 64, (SPLIT_SLOT, 4)),
    Contract("set_split_k_f16", "a", "f16", 2, 64, (SPLIT_SLOT, 4)),
    Contract("set_split_k_i8", "a", "i8", 2, 64, (SPLIT_SLOT, 2)),
    Contract("set_stem_fusion", "a", "f32", 3, 64, (0,)),
    Contract("set_stem_fusion_f16", "a", "f16", 3, 64, (1,)),
    Contract("set_k_chunk", "a", "f32", 3, 64, (32,)),
    Contract("set_border_skip", "a", "f32", BORDER_BATCH, BORDER_CANVAS, (1,)),
    Contract("set_xcd_mode", "a", "f32", 3, 64, (0,)),
)
WAITS_FOR_PLAN = (
    Contract("set_tiny_stem_fusion", "b", "f32", 2, 64, (True,)),
    Contract("set_early_chunk", "a", "f32", 5, 64, (4, 2)),
    Contract("keep_activations", "a", "f32", 3, 64, (True,)),
    Contract("set_act_scales", "a", "i8", 3, 64, ("other",)),
)
# y3_net_set_early_chunk on a net whose plan is chunked (9 convs, 2 images): the forward steps by the plan's chunk, never the live one
EARLY_PLANNED = (9, 2)
EARLY_CALLS = ((0, 0), (9, 0), (4, 16))

# ---------------------------------------------------------------------------------------------- refused plans
# (name, program, the refused plan as (max_batch, canvas, mode), outcome): "a" the old plan intact, "b" no plan in either layer
# (include/y3.h, the table at y3_net_plan_hw).  setup: what makes the call refusable.
Refusal = namedtuple("Refusal", "name net max_batch canvas mode outcome setup match")
HUGE_BATCH = 1 << 21       # program A at 32 x 32: conv 0's tensor is 2^21 * 32 * 32 * 32 * 4 bytes = 256 GiB, refused before any allocation
# (the two divisibility cases plan YOLOv3-tiny, whose largest div is 32, at a side of 40: no multiple of 32; the message names the first
# div that does not divide it, 16)
REFUSALS = (
    Refusal("side_not_divisible", "b", 2, 40, "f32", "a", None, "not divisible by"),
    Refusal("side_not_divisible_hw", "b", 2, (64, 40), "f32", "a", None, "not divisible by"),
    Refusal("tiny_f32x3", "b", 2, 64, "f32x3", "a", None, "max-pool"),
    Refusal("tiny_f32x2", "b", 2, 64, "f32x2", "a", None, "max-pool"),
    Refusal("tiny_i8", "b", 2, 64, "i8", "a", None, "max-pool"),
    Refusal("f32x2_weight_out_of_range", "a", 2, 64, "f32x2", "a", "bad_weights", "outside the fp16 range"),
    Refusal("i8_without_scales", "a", 2, 64, "i8", "b", None, "needs the scale"),
    Refusal("i8_no_qualifying_conv", "noi8", 2, 64, "i8", "b", None, "qualifies for int8"),
    Refusal("no_16bit_tile", "odd", 2, 64, "bf16", "b", None, "tile"),
    Refusal("four_gib_guard", "a", HUGE_BATCH, 32, "f32", "b", None, "4 GiB"),
)


def refusal_tensor_bytes(r):
    """Bytes of the largest fp32 tensor of the refused plan (the host test: the guard case is beyond 4 GiB, far beyond)."""
    p = program(r.net)
    h, w = canvas_hw(r.canvas)
    stored = list(p.stored) if p.stored else [t.channels for t in p.tensors]
    return max(r.max_batch * (h // t.div) * (w // t.div) * c * 4 for t, c in zip(p.tensors, stored))
