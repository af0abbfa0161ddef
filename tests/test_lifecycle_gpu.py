"""One long-lived Net through many plans against a freshly planned twin, bit for bit (tests/lifecycle_cases.py; the walks and the fold
are checked on the CPU by tests/test_lifecycle_host.py).  Nothing here is compared with a reference but the library with itself:
torch.equal on the head grids, on detect's packed rows and counts, and on read_tensor of every stored tensor.  No tolerance anywhere.

1. The walks: at every forward / detect / read step a fresh Net gets the folded settings, one plan with the long-lived net's
   (max_batch, image size, dtype) and the same lanes, runs the same call and is dropped.  Python's fields are held to the fold as well.
   A walk fails when the mechanism it is there to stress was never in force (lifecycle_cases.ENGAGEMENTS).
2. The contract of every setter on a planned net: acts at once, or waits for the next plan (include/y3.h, "Setters on a planned net").
3. y3_net_set_early_chunk on a net whose plan is chunked: the forward returns.
4. Refused plans leave the old plan intact or no plan in either layer (include/y3.h, the table at y3_net_plan_hw).
5. read_tensor and multi_label_totals right after a new plan."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import lifecycle_cases as L  # noqa: E402
from yolo_v3_tf2_amd._lib import Y3Error  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _feed(rt, key, mode, canvas, B):
    """The input batch in the form a plan of `mode` takes (a 3-channel image is fp32 in every mode)."""
    x = torch.from_numpy(np.array(L.images(key, canvas, B), order="C")).cuda()
    if x.shape[-1] == 3 or mode == "f32":
        return x
    if mode == "f32x3":
        return rt.split3_planes(x)
    if mode == "f32x2":
        return rt.split2_planes(x)
    return x.to(torch.bfloat16 if mode == "bf16" else torch.float16)


_scales = {}


def _calibration(rt, key, which="shared"):
    """One calibration per program, made once on a net of its own and handed to both sides through set_act_scales; "other": the same
    scales times 1.5, for the test that a planned int8 net does not follow set_act_scales."""
    if (key, "shared") not in _scales:
        net = rt.Net(L.program(key))
        net.load_weights(L.weights(key, 1))
        x = torch.from_numpy(np.array(L.images(key, 64, 4), order="C")).cuda()
        _scales[(key, "shared")] = tuple(net.calibrate_i8(x))
        _scales[(key, "other")] = tuple(1.5 * s for s in _scales[(key, "shared")])
    return _scales[(key, which)]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _scales.clear()


class Runner:
    """A long-lived net, the steps it has taken, and the twin on demand."""

    def __init__(self, rt, key):
        self.rt, self.key, self.p = rt, key, L.program(key)
        self.net = rt.Net(self.p)
        self.state = L.State()
        self.steps = []
        self.own_scales = {}
        self.engaged = set()
        self.checked = 0
        self.detect_steps, self.detections = 0, 0      # detect steps taken, and the valid rows they returned in all

    def scales(self, sid):
        if sid is None:
            return [0.0] * len(self.p.tensors)
        return self.own_scales[sid] if isinstance(sid, tuple) else _calibration(self.rt, self.key, sid)

    def _call(self, net, state, kind, B):
        x = _feed(self.rt, self.key, state.dtype, state.canvas, B)
        if kind == "forward":
            return net.forward(x)
        return list(net.detect(x, L.anchors(self.key), L.MAX_BOXES, L.IOU, L.SCORE))

    def twin(self, state=None, seed=None):
        state = state or self.state
        t = self.rt.Net(self.p)
        t.load_weights(L.weights(self.key, seed if seed is not None else state.seed))
        t.set_act_scales(self.scales(state.planned_scales))
        calls = L.twin_calls(state)
        for when, name, args in calls:
            if when == "before":
                getattr(t, name)(*args)
        t.plan(state.max_batch, state.image_size, L.DTYPE[state.dtype])
        for when, name, args in calls:
            if when == "after":
                getattr(t, name)(*args)
        for name, v in state.attrs.items():
            if self.p.nclasses > 0:
                setattr(t, name, v)
        return t

    def fields(self):
        """Python's fields against the fold."""
        n, s = self.net, self.state
        assert (n.max_batch, n.canvas, n.dtype) == (s.max_batch, s.canvas, L.DTYPE[s.dtype]), (len(self.steps), self.steps[-1])
        if s.max_batch:
            assert n.image_size == s.image_size and n.lanes == s.lanes, (len(self.steps), self.steps[-1], n.image_size, n.lanes)
            # grid_sizes() answers in the form of the plan (Net._plan_for): ints for an int plan, pairs for a pair plan
            assert all(isinstance(g, tuple) == isinstance(s.image_size, tuple) for g in n.grid_sizes())

    def note(self, B=None):
        n, s, e = self.net, self.state, self.engaged
        if not s.max_batch:
            return
        if n.tiny_stem_fused:
            e.add("tiny_stem")
        if n.i8_first_conv() not in (-1, 0):
            e.add("i8_cut")
        slots = range(len(n.conv_ops))
        for sfx in ("", "_bf16", "_f16", "_i8"):
            if any(getattr(n, "split_k" + sfx)(i) > 1 for i in slots):
                e.add("split" + (sfx or "_f32"))
        if n.lib.y3_net_get_early_chunk(n._h, None) > 0:
            e.add("early")
        if B is not None:
            if min(s.lanes, B) > 1:
                e.add("lanes")
            if any(n.border_skip(i, B) > 0 for i in slots):
                e.add("border")

    def read_all(self, net, B):
        out = {}
        for t in L.stored_tensors(self.p):
            try:
                out[t] = net.read_tensor(t, B)
            except Y3Error as err:      # a tensor inside the fused tiny stem is never stored: both sides must say so
                out[t] = str(err).split(":", 1)[-1]
        return out

    def step(self, s, check=True):
        """Take one step; a forward / detect / read is compared with the twin.  -> what the long-lived net returned."""
        self.steps.append(s)
        self.state.step(s, len(self.steps) - 1)
        kind, net = s[0], self.net
        got = None
        if kind == "plan":
            net.plan(s[1], s[2], None if s[3] is None else L.DTYPE[s[3]])
        elif kind == "set_dtype":
            net.set_dtype(s[1])
        elif kind == "set":
            getattr(net, s[1])(*s[2:])
        elif kind == "attr":
            setattr(net, s[1], s[2])
        elif kind == "load":
            net.load_weights(L.weights(self.key, s[1]))
        elif kind == "scales":
            net.set_act_scales(self.scales(s[1]))
        elif kind == "calibrate":
            x = torch.from_numpy(np.array(L.images(self.key, s[2], s[1]), order="C")).cuda()
            self.own_scales[("own", len(self.steps) - 1)] = tuple(net.calibrate_i8(x))
        elif kind in ("forward", "detect"):
            got = self._call(net, self.state, kind, s[1])
            self.fields()
            self.note(s[1])
            if check:
                twin = self.twin()
                want = self._call(twin, self.state, kind, s[1])
                assert len(got) == len(want)
                if kind == "detect":
                    self.detect_steps += 1
                    self.detections += int(got[1].sum())
                for k, (a, b) in enumerate(zip(got, want)):
                    assert _same(a, b), f"step {len(self.steps) - 1} {s}: output {k} differs from the freshly planned net's"
                self.checked += 1
        elif kind == "read":
            assert self.state.planned["keep_activations"] == (True,) and self.state.last, "a read step needs a kept plan and a forward"
            lk, B = self.state.last
            twin = self.twin()
            self._call(twin, self.state, lk, B)
            got, want = self.read_all(net, B), self.read_all(twin, B)
            for t in got:
                same = got[t] == want[t] if isinstance(got[t], str) or isinstance(want[t], str) else _same(got[t], want[t])
                assert same, f"step {len(self.steps) - 1}: stored tensor {t} differs from the freshly planned net's"
            self.checked += 1
        self.fields()
        self.note()
        return got


# ---------------------------------------------------------------------------------------------- 1. the walks
@pytest.mark.parametrize("walk", L.WALKS, ids=[w.name for w in L.WALKS])
def test_walk_equals_the_freshly_planned_twin(rt, walk):
    r = Runner(rt, walk.net)
    for s in walk.steps:
        r.step(s)
    torch.cuda.synchronize()
    assert r.checked >= 2
    # equal EMPTY detections would say nothing about the NMS mode or the multi-label route of the long-lived net
    assert r.detect_steps == 0 or r.detections >= r.detect_steps, (r.detect_steps, r.detections)
    missing = set(walk.needs) - r.engaged
    assert not missing, f"walk {walk.name} never had {sorted(missing)} in force (engaged: {sorted(r.engaged)})"
    print(f"walk {walk.name}: {len(walk.steps)} steps, {r.checked} checked against a twin, engaged {sorted(r.engaged)}")


def test_reload_out_of_range_weights_under_an_f32x2_plan(rt):
    """Weights with a BN-scaled value beyond 65504 loaded on a planned two-plane net: the forward refuses by name; good weights loaded
    afterwards run and equal a twin that only ever saw them."""
    r = Runner(rt, "a")
    for s in (("load", 1), ("plan", 2, 64, "f32x2"), ("forward", 2)):
        r.step(s)
    r.net.load_weights(L.out_of_range_weights("a", 1))
    with pytest.raises(Y3Error, match="outside the fp16 range"):
        r._call(r.net, r.state, "forward", 2)
    for s in (("load", 2), ("forward", 2)):
        r.step(s)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. the setters' contract
def _planned(rt, c, pre=()):
    r = Runner(rt, c.net)
    for s in (("load", 1), ("scales", "shared" if c.mode == "i8" else None)) + tuple(pre) + (("plan", c.max_batch, c.canvas, c.mode),):
        r.step(s)
    return r


@pytest.mark.parametrize("c", L.ACTS_AT_ONCE, ids=[c.name for c in L.ACTS_AT_ONCE])
def test_setter_acts_at_once_on_a_planned_net(rt, c):
    """plan, forward, the setter, forward: the second forward equals a twin configured that way before its single plan.  Where
    include/y3.h says the setting changes the bits (lifecycle_cases.MUST_DIFFER) the second forward must differ from the first, so the
    twin it equals is not the first forward's."""
    r = _planned(rt, c)
    B = c.max_batch
    before = r.step(("forward", B))
    r.step(("set", c.name) + tuple(c.args))
    after = r.step(("forward", B))
    if c.name in L.MUST_DIFFER:
        assert not all(_same(a, b) for a, b in zip(before, after)), f"{c.name}{c.args} on the planned net changed nothing"
    if B > 1:
        r.step(("forward", B - 1))
    torch.cuda.synchronize()
    if c.name.startswith(("set_split_k", "set_low_latency")):
        sfx = c.name[len("set_split_k"):] if c.name.startswith("set_split_k") else c.name[len("set_low_latency"):]
        forced = c.name.startswith("set_split_k")
        in_force = max(getattr(r.net, "split_k" + sfx)(i) for i in range(len(r.net.conv_ops)))
        # the int8 rule's floor of 36 K tiles of 128 (K >= 4608) is beyond every conv of a program under the weight budget: the switch
        # is in force, and changes nothing
        assert in_force > 1 or (not forced and sfx == "_i8"), (c.name, in_force)
    if c.name == "set_border_skip":
        assert "border" in r.engaged
    if c.name == "set_lanes":
        assert "lanes" in r.engaged


@pytest.mark.parametrize("c", L.WAITS_FOR_PLAN, ids=[c.name for c in L.WAITS_FOR_PLAN])
def test_setter_waits_for_the_next_plan(rt, c):
    """plan, forward, the setter, forward: the bits of the forward before the call (and of a twin that never saw it).  After a new plan
    the net equals a twin configured with the new value."""
    r = _planned(rt, c)
    B = c.max_batch
    before = r.step(("forward", B))
    if c.name == "set_act_scales":
        r.step(("scales", c.args[0]))
    else:
        r.step(("set", c.name) + tuple(c.args))
    after = r.step(("forward", B))
    assert all(_same(a, b) for a, b in zip(before, after)), f"{c.name} changed the planned net's results before a new plan"
    r.step(("plan", c.max_batch, c.canvas, c.mode))
    fresh = r.step(("forward", B))
    torch.cuda.synchronize()
    if c.name == "set_tiny_stem_fusion":
        assert "tiny_stem" in r.engaged
    if c.name == "set_early_chunk":
        assert "early" in r.engaged
    if c.name == "set_act_scales":
        assert not all(_same(a, b) for a, b in zip(before, fresh)), "other scales, the same int8 results: the test's scales do nothing"
    if c.name == "keep_activations":
        r.step(("read",))


# ---------------------------------------------------------------------------------------------- 3. set_early_chunk on a chunked plan
@pytest.mark.parametrize("call", L.EARLY_CALLS, ids=[f"{a}_{b}" for a, b in L.EARLY_CALLS])
def test_set_early_chunk_on_a_chunked_plan_returns(rt, call):
    """On a net planned with set_early_chunk(9, 2): the setter call, then a forward.  The forward steps through the chunked segment by the
    plan's own chunk size (csrc/y3_forward.cpp, run_lane), so it returns, with the bits of the forward before the call; a new plan then
    equals a twin configured with the call's values (unchunked for (0, 0) and (9, 0))."""
    r = Runner(rt, "a")
    for s in (("load", 1), ("set", "set_early_chunk") + L.EARLY_PLANNED, ("plan", 5, 64, "f32")):
        r.step(s)
    chunk = C.c_int()
    assert r.net.lib.y3_net_get_early_chunk(r.net._h, C.byref(chunk)) > 0 and chunk.value == L.EARLY_PLANNED[1]
    before = r.step(("forward", 5))
    r.step(("set", "set_early_chunk") + tuple(call))
    assert r.net.lib.y3_net_get_early_chunk(r.net._h, C.byref(chunk)) > 0 and chunk.value == L.EARLY_PLANNED[1]
    after = r.step(("forward", 5))
    assert all(_same(a, b) for a, b in zip(before, after))
    r.step(("plan", 5, 64, "f32"))
    chunked = r.net.lib.y3_net_get_early_chunk(r.net._h, C.byref(chunk)) > 0
    assert chunked == (call[0] > 0 and call[1] > 0) and chunk.value == (call[1] if chunked else 0)
    r.step(("forward", 5))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 4. refused plans
def _refused_call(r, ref, route):
    """Make the refused call through `route`; -> the error text."""
    net = r.net
    with pytest.raises(Y3Error) as err:
        if route == "plan":
            net.plan(ref.max_batch, ref.canvas, L.DTYPE[ref.mode])
        elif route == "set_dtype":
            net.set_dtype(ref.mode)
        else:      # a forward whose shape the plan does not fit: _plan_for plans
            h, w = L.canvas_hw(ref.canvas)
            net.forward(torch.zeros((ref.max_batch, h, w, 3), dtype=torch.float32, device="cuda"))
    return str(err.value)


def _routes(ref):
    routes = ["plan"]
    if ref.mode != "f32" and ref.max_batch == 2 and ref.canvas == 64:
        routes.append("set_dtype")          # the same batch and canvas in another mode: what set_dtype plans
    if ref.name.startswith("side_not_divisible"):
        routes.append("forward")
    return routes


def _refused_through_plan_for(rt, ref):
    """A mode's refusal reached through a forward: plan() makes its mode the net's dtype, so only a net that was never planned can hold
    another default -- set_dtype on it plans nothing, the forward's _plan_for does.  No plan before, none after, in either layer; the
    dtype the caller set stays; after set_dtype("f32") the forward plans by itself and equals the twin."""
    r = Runner(rt, ref.net)
    r.step(("load", 1))
    if ref.setup == "bad_weights":
        r.net.load_weights(L.out_of_range_weights(ref.net, 1))
    r.step(("set_dtype", ref.mode))
    net = r.net
    with pytest.raises(Y3Error) as err:
        net.forward(_feed(rt, ref.net, ref.mode, ref.canvas, ref.max_batch))
    assert ref.match in str(err.value), str(err.value)
    assert net.lib.y3_net_get_plan(net._h, None, None, None, None) == 0
    assert (net.max_batch, net.canvas, net.dtype) == (0, (0, 0), L.DTYPE[ref.mode]), ref.name
    if ref.setup == "bad_weights":
        r.step(("load", 1))
    r.step(("set_dtype", "f32"))
    r.step(("forward", 2, 64))
    torch.cuda.synchronize()


@pytest.mark.parametrize("ref", L.REFUSALS, ids=[r.name for r in L.REFUSALS])
def test_refused_plan_leaves_the_old_plan_or_none(rt, ref):
    """A working fp32 plan and a forward; then the refused call, through Net.plan, through set_dtype where the refusal is a mode's, and
    through a forward of another shape where it is a shape's; a mode's refusal also through the forward of a net that was never planned
    (_refused_through_plan_for).  The 4 GiB case has the one route: its forward would take 2^21 images.  (a) the old plan is intact: Python's fields unchanged, the next forward
    has the bits of the one before.  (b) no plan in either layer: max_batch 0, canvas (0, 0), dtype unchanged, y3_net_get_plan 0; the
    next forward plans by itself and equals the twin."""
    if ref.mode != "f32":
        _refused_through_plan_for(rt, ref)
    for route in _routes(ref):
        r = Runner(rt, ref.net)
        for s in (("load", 1), ("plan", 2, 64, "f32")):
            r.step(s)
        before = r.step(("forward", 2))
        if ref.setup == "bad_weights":
            r.net.load_weights(L.out_of_range_weights(ref.net, 1))
            before = r._call(r.net, r.state, "forward", 2)      # fp32 runs them
        text = _refused_call(r, ref, route)
        assert ref.match in text, text
        net = r.net
        planned = net.lib.y3_net_get_plan(net._h, None, None, None, None)
        if ref.outcome == "a":
            assert planned == 1
            r.fields()
            after = r._call(net, r.state, "forward", 2)
            assert all(_same(a, b) for a, b in zip(before, after)), (ref.name, route)
        else:
            assert planned == 0
            assert (net.max_batch, net.canvas, net.dtype) == (0, (0, 0), L.DTYPE["f32"]), (ref.name, route)
            with pytest.raises(Y3Error):
                net.read_tensor(1, 1)
            r.state = L.fold(r.steps[:1])           # the fold of a net that was never planned, with its weights
            after = r.step(("forward", 2, 64))      # plans by itself; compared with the twin
            assert all(_same(a, b) for a, b in zip(before, after)), (ref.name, route)
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 5. read-backs right after a new plan
def test_read_backs_right_after_a_new_plan_are_refused(rt):
    """read_tensor (the read, not the size query) and multi_label_totals between a new plan and the first forward / detect on it: the
    previous plan's data is gone, Y3_ERR_STATE (-4) says so; after a forward / detect on the new plan both answer."""
    r = Runner(rt, "a")
    for s in (("load", 1), ("set", "keep_activations", True), ("plan", 3, 64, "f32"), ("attr", "multi_label", True), ("detect", 3)):
        r.step(s)
    t = L.stored_tensors(r.p)[2]
    assert r.net.read_tensor(t, 3).shape[0] == 3 and r.net.multi_label_totals.shape == (3,)
    for replan in (("plan", 3, 64, "f32"), ("plan", 2, 32, "bf16"), ("set_dtype", "f16")):
        r.step(replan)
        n = C.c_size_t()
        assert r.net.lib.y3_net_read_tensor(r.net._h, t, 1, None, C.byref(n), None) == 0 and n.value > 0      # the size query stays
        with pytest.raises(Y3Error, match=r"\(-4\).*no forward was enqueued on this plan"):
            r.net.read_tensor(t, 1)
        with pytest.raises(Y3Error, match=r"\(-4\).*no multi-label"):
            r.net.multi_label_totals
        r.step(("detect", 2))
        assert r.net.read_tensor(t, 2).shape[0] == 2 and r.net.multi_label_totals.shape[0] == r.net.max_batch
    r.step(("read",))
    torch.cuda.synchronize()
