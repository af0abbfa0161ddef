"""The basis of tests/test_lifecycle_gpu.py, checked without a GPU (tests/lifecycle_cases.py): the mode walk takes every ordered pair of
modes once, every setter of Net occurs in the walks before a plan and on a planned net, the settings fold follows the survival rules
the docstrings state, the reduced programs are what the walks need, and every step stays within the sizes a twin per step can afford."""
import os
import re

from tests import lifecycle_cases as L
from tests.test_runtime_surface_host import NET_METHODS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrivals(walk):
    """[(mode before, mode after)] of every step of a walk that changes the planned mode."""
    st, out = L.State(), []
    for i, s in enumerate(walk.steps):
        was = st.dtype if st.max_batch else None
        st.step(s, i)
        if s[0] in ("plan", "set_dtype") and was is not None and st.dtype != was:
            out.append((was, st.dtype))
    return out


def test_mode_walk_takes_each_ordered_pair_exactly_once():
    tour = L.euler_circuit()
    pairs = list(zip(tour, tour[1:]))
    want = {(a, b) for a in L.MODES for b in L.MODES if a != b}
    assert len(pairs) == 30 and set(pairs) == want and tour[0] == tour[-1]
    arrivals = _arrivals(L.mode_walk())
    assert sorted(arrivals) == sorted(want), "the walk's plans and set_dtypes are not the circuit"
    # every arrival is followed by a checked forward before the next transition, and both transition kinds occur
    steps = L.mode_walk().steps
    kinds = [s[0] for s in steps if s[0] in ("plan", "set_dtype", "forward")]
    assert re.fullmatch(r"(?:[ps]f)+", "".join({"plan": "p", "set_dtype": "s", "forward": "f"}[k] for k in kinds))
    assert kinds.count("set_dtype") >= 8 and kinds.count("plan") >= 16
    assert {s[2] if s[0] == "plan" else None for s in steps} >= set(L.CANVASES)
    assert {s[2] for s in steps if s[0] == "set" and s[1] == "set_lanes"} == {1, 2, 3}


def test_every_setter_occurs_before_a_plan_and_on_a_planned_net():
    """In the walks alone: every set_* of Net, keep_activations and set_tiny_stem_fusion is called on a net that was never planned and
    on a planned net, or is named in SETTER_EXEMPT with its reason.  Every one has a contract test besides."""
    setters = sorted(n for n in NET_METHODS if n.startswith("set_")) + ["keep_activations", "set_tiny_stem_fusion"]
    before, planned = set(), set()
    for w in L.WALKS:
        st = L.State()
        for i, s in enumerate(w.steps):
            if s[0] == "set":
                (planned if st.max_batch else before).add(s[1])
            st.step(s, i)
    for name in setters:
        if name in L.SETTER_EXEMPT:
            assert L.SETTER_EXEMPT[name].strip()
            continue
        assert name in planned, f"{name} is never called on a planned net"
        assert name in before, f"{name} is never called before a first plan"
    assert set(L.SETTER_EXEMPT) <= set(setters)
    # the two exempt ones have step kinds of their own, and those occur on both sides as well
    for kind in ("set_dtype", "scales"):
        sides = set()
        for w in L.WALKS:
            st = L.State()
            for i, s in enumerate(w.steps):
                if s[0] == kind:
                    sides.add(bool(st.max_batch))
                st.step(s, i)
        assert sides == {False, True}, kind
    assert {c.name for c in L.ACTS_AT_ONCE} | {c.name for c in L.WAITS_FOR_PLAN} | {"set_dtype"} == set(setters), \
        "a setter of Net has no contract test"
    assert set(L.MUST_DIFFER) <= {c.name for c in L.ACTS_AT_ONCE}


def test_twin_configures_before_its_plan_and_lanes_after():
    st = L.fold((("set", "set_tile", 4, 11), ("plan", 2, 64, "f32"), ("set", "set_lanes", 2), ("set", "set_k_chunk", 32),
                 ("set", "set_split_k", 10, 3)))
    calls = L.twin_calls(st)
    assert [c for c in calls if c[0] == "after"] == [("after", "set_lanes", (2,))]
    assert {c[1] for c in calls if c[0] == "before"} >= {"set_tile", "set_k_chunk", "set_split_k", "keep_activations",
                                                          "set_early_chunk", "set_tiny_stem_fusion"}


def test_fold_survival_rules():
    """Hand-written expectations: forced tiles survive plans and are released by -1; lanes are reset by every plan (the tuning table's,
    1 without a table); the dtype default follows plan() and set_dtype() and calibrate_i8 leaves it at fp32; the four setters that wait
    are taken by the next plan only; _plan_for grows max_batch only and keeps the form of the plan."""
    f = L.fold
    st = f((("set", "set_tile", 4, 11), ("plan", 2, 64, "bf16"), ("plan", 3, 32, "f32")))
    assert st.tiles == {("", 4): 11} and (st.max_batch, st.image_size, st.dtype) == (3, 32, "f32")
    assert f((("set", "set_tile", 4, 11), ("plan", 2, 64, "f32"), ("set", "set_tile", 4, -1))).tiles == {}
    assert f((("set", "set_split_k_bf16", 10, 4), ("plan", 2, 64, "f32"), ("set", "set_split_k_bf16", 10, -1))).splits == {}
    st = f((("plan", 4, 64, "f32"), ("set", "set_lanes", 3)))
    assert st.lanes == 3
    assert f((("plan", 4, 64, "f32"), ("set", "set_lanes", 3), ("plan", 4, 64, "f32"))).lanes == 1
    assert f((("set", "set_lanes", 3), ("forward", 2, 64))).lanes == 1, "_plan_for plans: the tuning table's lanes"
    assert f((("plan", 4, 64, "f32"), ("set", "set_lanes", 3), ("forward", 5))).lanes == 1
    assert f((("plan", 4, 64, "f32"), ("set", "set_lanes", 3), ("forward", 4))).lanes == 3
    assert L.table_lanes("bf16", 64, 416) >= 1 and L.table_lanes("f32", 3, 64) == 1
    # dtype default
    assert f((("plan", 2, 64, "bf16"), ("plan", 2, 32, None))).dtype == "bf16"
    assert f((("set_dtype", "f16"), ("forward", 2, 64))).dtype == "f16"
    st = f((("set_dtype", "i8"), ("calibrate", 2, 32)))
    assert (st.dtype, st.image_size, st.max_batch) == ("f32", (32, 32), 2)
    assert st.planned["keep_activations"] == (True,) and st.pending["keep_activations"] == (False,)
    assert st.pending_scales == ("own", 1) and st.planned_scales is None
    st = f((("plan", 2, 64, "f32"), ("set_dtype", "bf16")))
    assert (st.max_batch, st.image_size, st.dtype) == (2, 64, "bf16")
    # the setters that wait
    st = f((("plan", 2, 64, "f32"), ("set", "set_early_chunk", 4, 2), ("set", "keep_activations", True),
            ("set", "set_tiny_stem_fusion", True), ("scales", "shared")))
    assert st.planned == L.AT_PLAN and st.planned_scales is None
    st.step(("forward", 2))
    assert st.planned == L.AT_PLAN
    st.step(("forward", 3))
    assert st.planned == {"set_early_chunk": (4, 2), "keep_activations": (True,), "set_tiny_stem_fusion": (True,)}
    assert st.planned_scales == "shared"
    # growth and form (Net._plan_for)
    st = f((("forward", 2, 64), ("forward", 5, 64), ("forward", 3, 64)))
    assert (st.max_batch, st.image_size) == (5, 64)
    st.step(("forward", 2, (64, 96)))
    assert (st.max_batch, st.image_size) == (5, (64, 96))
    st.step(("forward", 4, 64))
    assert (st.max_batch, st.image_size) == (5, (64, 64)), "a net planned with a pair stays a pair plan also for an H == W batch"
    assert f((("plan", 2, (64, 64), "f32"), ("forward", 2, 32))).image_size == (32, 32)
    # attrs and at-once setters: last call wins, plans change nothing
    st = f((("attr", "nms_per_class", True), ("set", "set_k_chunk", 32), ("plan", 1, 32, "f32"), ("set", "set_k_chunk", 0)))
    assert st.attrs == {"nms_per_class": True, "multi_label": False} and st.simple == {"set_k_chunk": (0,)}


def test_reduced_programs():
    from yolo_v3_tf2_amd import quant
    for key in ("a", "a80", "c"):
        p = L.program(key)
        assert L.n_weights(p) < L.WEIGHT_BUDGET, (key, L.n_weights(p))
    for key in ("a", "a80"):
        p = L.program(key)
        convs = p.conv_ops()
        stem = [(o.cin, o.cout, o.size, o.stride, o.residual >= 0) for o in convs[:4]]
        assert stem == [(3, 32, 3, 1, False), (32, 64, 3, 2, False), (64, 32, 1, 1, False), (32, 64, 3, 1, True)]
        cut = quant.first_i8_conv(p)
        assert 0 < cut < len(convs) - 1 and cut == 7
        behind = {o.dst for o in convs[cut:]}
        crossing = {t for o in convs[cut:] for t in (o.src0, o.src1, o.residual) if t >= 0 and t not in behind}
        assert crossing, "no tensor crosses the int8 cut"
        assert len(p.outputs) == 2 and any(o.src0_upsample for o in convs), "the folding upsample + route is gone"
        o = convs[L.SPLIT_SLOT]
        assert (o.cin, o.cout, o.size) == (256, 128, 3) and o.dst not in p.outputs and o.size * o.size * o.cin // 64 >= 32
        for t in L.CANVASES:
            assert all(v % max(x.div for x in p.tensors) == 0 for v in L.canvas_hw(t))
    assert L.program("a").nclasses == 5 and L.program("a80").nclasses == 80
    assert quant.first_i8_conv(L.program("noi8")) == -1
    from yolo_v3_tf2_amd.graph import AuxOp
    assert any(isinstance(o, AuxOp) and o.kind == "add" for o in L.program("c").ops), "program C lost its stand-alone add"


def test_every_step_is_small():
    """At most 7 images of at most 96 x 96 per step -- but for the one border-skip geometry, 32 images of 32 x 32 (fewer pixels than
    four images at 96 x 96): the border skip takes whole blocks of 32 images and cannot be in force below that."""
    def ok(B, canvas):
        h, w = L.canvas_hw(canvas)
        return (B <= L.MAX_IMAGES and max(h, w) <= L.MAX_SIDE) or (B, canvas) == (L.BORDER_BATCH, L.BORDER_CANVAS)
    for w in L.WALKS:
        st = L.State()
        for i, s in enumerate(w.steps):
            st.step(s, i)
            if st.max_batch:
                assert ok(st.max_batch, st.image_size), (w.name, i, s)
        assert set(w.needs) <= set(L.ENGAGEMENTS)
        assert w.net in L.PROGRAM_MODES and all(s[3] in L.PROGRAM_MODES[w.net] + (None,) for s in w.steps if s[0] == "plan")
    for c in L.ACTS_AT_ONCE + L.WAITS_FOR_PLAN:
        assert ok(c.max_batch, c.canvas) and c.mode in L.PROGRAM_MODES[c.net]
    assert {e for w in L.WALKS for e in w.needs} == set(L.ENGAGEMENTS), "an engagement condition no walk asks for"


def test_refusal_table_matches_the_header():
    """Every refusal of the table has its outcome named at y3_net_plan_hw in include/y3.h and in DESIGN.md; the 4 GiB case is beyond the
    guard by construction, not by allocation."""
    header = open(os.path.join(ROOT, "include", "y3.h")).read()
    at = header.index("A refused or failed call on a planned net leaves one of two states")
    table = header[at:header.index("y3_status y3_net_plan_hw", at)]
    assert table.count("(a)") >= 5 and table.count("(b)") >= 6 and "hipGraph" in table
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "y3_net_get_plan" in design and "Refused plans" in design
    assert {r.outcome for r in L.REFUSALS} == {"a", "b"}
    guard = [r for r in L.REFUSALS if r.name == "four_gib_guard"][0]
    assert L.refusal_tensor_bytes(guard) >= 1 << 36
    assert all(L.refusal_tensor_bytes(r) < 1 << 26 for r in L.REFUSALS if r is not guard)
