"""Decode inputs the N(0, 1.5) grids of the parity suite never produce, shared by tests/test_decode_edges_host.py (the CPU reference
holds what each case claims) and tests/test_decode_edges_gpu.py (decode_kernel / class_scores_kernel against it): class counts from 1
to 81 (lanes of a box that hold no class, every remainder of nc mod 4), tied class probabilities (equal logits, and different logits
that saturate to the same 1.0f or 0.0f), and saturated objectness / centre / size fields (exp(tw) * anchor overflowing to inf).

A case is a dict: name, nc, gs (three (gh, gw)), grids (three fp32 [B, gh, gw, 3, 5 + nc]) and what is expected of them, every
entry in output order [B, N] (n = off_s + (row * gw + col) * 3 + a):
  cls         int64 [B, N]   the class index of every box, or None where the case claims none (random logits)
  score_conf  bool  [B, N]   score == objectness, bit for bit (the winning probability is exactly 1.0f)
  score_zero  bool  [B, N]   score is exactly 0.0f
  conf_one / conf_zero  bool [B, N]       objectness exactly 1.0f / 0.0f
  prob_one / prob_zero  bool [B, N, nc]   class probability exactly 1.0f / 0.0f
  box_inf     int8  [B, N, 4]  +1 / -1 where the coordinate is +inf / -inf, 0 where it is finite
  wh_zero     bool  [B, N, 2]  width / height exactly 0: box[0] == box[2] / box[1] == box[3] bit for bit

Two grid sets, one seed.  SQUARE = (2, 4, 8); RECT = ((1, 3), (2, 6), (4, 12)).  decode_kernel takes 64 boxes of one scale per
workgroup and copies them as 16-byte vectors plus a scalar tail.  With B = 3 the scales hold 36 / 144 / 576 boxes (SQUARE: the last
workgroup of the first two scales is partial, the third scale is nine full workgroups, and every nbox * F is a multiple of four) and
27 / 108 / 432 boxes (RECT: the last workgroup of every scale is partial, and the 27 boxes of the first scale leave a scalar tail
of 1 to 3 floats whenever (5 + nc) % 4 != 0).  tests/test_decode_edges_host.py asserts exactly that.

Saturation, fp32, sigmoid(x) = 1 / (1 + expf(-x)): every logit above about 16.7 gives exactly 1.0f (expf(-x) < 2^-24), every
logit below -88.8 gives exactly 0.0f once expf(-x) is inf; expf(t) is inf above 88.8 and exactly 0 below about -104.
RANGE TO AVOID: no constructed logit lies in (-104, -87).  There the sigmoid (or expf) is a subnormal or on its edge: whether the
device keeps it depends on the denormal mode, the CPU oracle keeps it, TensorFlow on a GPU would not -- nothing pins the answer, so
no case asserts on that range (in_avoided_range, checked on every case by the host tier)."""
import itertools

import numpy as np

SEED = 31
SQUARE = ((2, 2), (4, 4), (8, 8))
RECT = ((1, 3), (2, 6), (4, 12))
GRID_SETS = {"square": SQUARE, "rect": RECT}
DEC_BOXES = 64                                  # boxes per workgroup of decode_kernel (csrc/decode.hip)
AVOID = (-104.0, -87.0)

CLASS_COUNTS = (1, 2, 3, 4, 5, 6, 37, 79, 81)
CLASS_COUNTS_BATCH = 3
TIED_COUNTS = (1, 3, 4, 7, 80)
TIED_KINDS = ("equal", "plus30", "minus110")
LIMIT_F = 640                                   # 64 boxes x 640 floats = 160 KB of LDS: the largest row launch_decode admits
LIMIT_GS = ((1, 1), (2, 2), (4, 4))


def n_boxes(gs):
    return 3 * sum(gh * gw for gh, gw in gs)


def in_avoided_range(grids):
    return any(bool(((g > AVOID[0]) & (g < AVOID[1])).any()) for g in grids)


def _rows(rng, B, gs, nc):
    """Random N(0, 1.5) logits as [B, N, 5 + nc] in output order."""
    return rng.normal(0, 1.5, (B, n_boxes(gs), 5 + nc)).astype(np.float32)


def _split(rows, gs):
    B, _, F = rows.shape
    out, off = [], 0
    for gh, gw in gs:
        n = gh * gw * 3
        out.append(np.ascontiguousarray(rows[:, off:off + n].reshape(B, gh, gw, 3, F)))
        off += n
    return out


def _case(name, rows, gs, nc, cls=None, **masks):
    B, N, _ = rows.shape
    c = dict(name=name, nc=nc, gs=gs, grids=_split(rows, gs), cls=cls,
             score_conf=np.zeros((B, N), bool), score_zero=np.zeros((B, N), bool),
             conf_one=np.zeros((B, N), bool), conf_zero=np.zeros((B, N), bool),
             prob_one=np.zeros((B, N, nc), bool), prob_zero=np.zeros((B, N, nc), bool),
             box_inf=np.zeros((B, N, 4), np.int8), wh_zero=np.zeros((B, N, 2), bool))
    for k, v in masks.items():
        assert c[k].shape == v.shape, k
        c[k] = v
    return c


# ---------------------------------------------------------------------------------------------- 1. class counts
def class_counts(gs, nc):
    rng = np.random.default_rng(SEED + nc)
    return _case(f"class_counts_nc{nc}", _rows(rng, CLASS_COUNTS_BATCH, gs, nc), gs, nc)


def workgroup_shape(gs, B, nc):
    """Per scale: (boxes of the scale over the batch, boxes of its last workgroup, floats of that workgroup's scalar tail)."""
    out = []
    for gh, gw in gs:
        total = B * gh * gw * 3
        last = total - (total - 1) // DEC_BOXES * DEC_BOXES
        out.append((total, last, last * (5 + nc) % 4))
    return out


# ---------------------------------------------------------------------------------------------- 2. ties between two classes
PAIR_NC = 9
PAIRS = tuple(itertools.combinations(range(PAIR_NC), 2))      # 36 pairs i < j: same lane (j - i = 4, 8), neighbours, two apart


def pair_ties(gs):
    """All class logits -3; 72 boxes at seeded places over both images and all scales: for each pair i < j one box where the two
    hold 18 + i and 18 + j (different logits, both exactly 1.0f) and one where both hold 0.75.  Class i in all 72, 0 elsewhere."""
    B, nc = 2, PAIR_NC
    rng = np.random.default_rng(SEED)
    rows = _rows(rng, B, gs, nc)
    rows[..., 5:] = -3.0
    N = rows.shape[1]
    places = rng.permutation(B * N)[:2 * len(PAIRS)]
    cls = np.zeros((B, N), np.int64)
    score_conf = np.zeros((B, N), bool)
    prob_one = np.zeros((B, N, nc), bool)
    for k, (i, j) in enumerate(PAIRS):
        b, n = divmod(int(places[2 * k]), N)
        rows[b, n, 5 + i], rows[b, n, 5 + j] = 18.0 + i, 18.0 + j
        cls[b, n] = i
        score_conf[b, n] = True
        prob_one[b, n, i] = prob_one[b, n, j] = True
        b, n = divmod(int(places[2 * k + 1]), N)
        rows[b, n, 5 + i] = rows[b, n, 5 + j] = 0.75
        cls[b, n] = i
    return _case("pair_ties", rows, gs, nc, cls=cls, score_conf=score_conf, prob_one=prob_one)


# ---------------------------------------------------------------------------------------------- 3. every class tied
def all_tied(gs, nc, kind):
    """Every class logit of every box equal (a value of the box's own), +30 (every probability 1.0f: score == objectness) or
    -110 (every probability 0.0f: score 0.0f).  Class 0 throughout."""
    B = 2
    rng = np.random.default_rng(SEED + 100 * nc + TIED_KINDS.index(kind))
    rows = _rows(rng, B, gs, nc)
    N = rows.shape[1]
    masks = {}
    if kind == "equal":
        rows[..., 5:] = rows[..., 5:6].copy()
    elif kind == "plus30":
        rows[..., 5:] = 30.0
        masks = dict(score_conf=np.ones((B, N), bool), prob_one=np.ones((B, N, nc), bool))
    else:
        assert kind == "minus110"
        rows[..., 5:] = -110.0
        masks = dict(score_zero=np.ones((B, N), bool), prob_zero=np.ones((B, N, nc), bool))
    return _case(f"all_tied_nc{nc}_{kind}", rows, gs, nc, cls=np.zeros((B, N), np.int64), **masks)


# ---------------------------------------------------------------------------------------------- 4. saturated fields
SAT_NC = 3
# (tx, ty, tw, th, objectness); None keeps the random logit
SATURATED = tuple(
    [(None, None, None, None, o) for o in (30.0, -110.0)]
    + [(x, y, None, None, None) for x in (30.0, -30.0) for y in (30.0, -30.0)]
    + [(None, None, w, h, None) for w in (100.0, -110.0, 10.0) for h in (100.0, -110.0, 10.0)]
    + [(None, None, 100.0, None, None), (None, None, None, 100.0, None), (30.0, -30.0, 100.0, -110.0, 30.0),
       (-30.0, 30.0, -110.0, 100.0, -110.0), (30.0, 30.0, 100.0, 100.0, 30.0)])


def saturated_fields(gs):
    """One box per row of SATURATED (twice over: seeded places in both images).  tw = 100: expf = inf, the box is
    [-inf, y, +inf, y]; tw = -110: the width is exactly 0; tw = 10: about 22026 anchors wide, finite.  No coordinate is NaN: the
    centre is always finite."""
    B, nc = 2, SAT_NC
    rng = np.random.default_rng(SEED + 7)
    rows = _rows(rng, B, gs, nc)
    N = rows.shape[1]
    places = rng.permutation(B * N)[:2 * len(SATURATED)]
    m = dict(score_zero=np.zeros((B, N), bool), score_conf=np.zeros((B, N), bool), conf_one=np.zeros((B, N), bool),
             conf_zero=np.zeros((B, N), bool), box_inf=np.zeros((B, N, 4), np.int8), wh_zero=np.zeros((B, N, 2), bool))
    for k, place in enumerate(places):
        b, n = divmod(int(place), N)
        tx, ty, tw, th, o = SATURATED[k % len(SATURATED)]
        for f, v in enumerate((tx, ty, tw, th, o)):
            if v is not None:
                rows[b, n, f] = v
        m["conf_one"][b, n] = o == 30.0
        m["conf_zero"][b, n] = m["score_zero"][b, n] = o == -110.0
        for axis, t in enumerate((tw, th)):
            if t == 100.0:
                m["box_inf"][b, n, axis], m["box_inf"][b, n, axis + 2] = -1, 1
            m["wh_zero"][b, n, axis] = t == -110.0
    return _case("saturated_fields", rows, gs, nc, **m)


# ---------------------------------------------------------------------------------------------- 5. the widest row
def limit_case(F=LIMIT_F):
    nc = F - 5
    rng = np.random.default_rng(SEED + 9)
    return _case(f"limit_F{F}", _rows(rng, 1, LIMIT_GS, nc), LIMIT_GS, nc)


def all_cases(gs):
    out = [class_counts(gs, nc) for nc in CLASS_COUNTS]
    out.append(pair_ties(gs))
    out += [all_tied(gs, nc, kind) for nc in TIED_COUNTS for kind in TIED_KINDS]
    out.append(saturated_fields(gs))
    return out


def case_ids():
    return [c["name"] for c in all_cases(SQUARE)]


# ---------------------------------------------------------------------------------------------- the CPU reference
_ref_cache = {}


def reference(case, anchors):
    """(boxes [B,N,4], conf [B,N], probs [B,N,nc], cls [B,N] i64, scores [B,N]) of a case on the CPU, computed once per case and
    left unchanged: oracle.yolo_decode on square grids; on gh != gw grids core/yolo_decode_layer.yolo_decode_hw_host, the NumPy
    restatement of the per-axis normalisation (the C oracle divides x by the number of rows there, as the reference does);
    y3o_scores for the first-maximum arg-max and the score either way."""
    key = (case["name"], case["gs"])
    if key not in _ref_cache:
        from oracle import oracle as O
        nc = case["nc"]
        if all(gh == gw for gh, gw in case["gs"]):
            rb, rc, rp = O.yolo_decode(case["grids"], anchors, nc)
        else:
            from yolo_v3_tf2_amd.core.yolo_decode_layer import yolo_decode_hw_host
            with np.errstate(over="ignore", invalid="ignore"):
                rb, rc, rp = yolo_decode_hw_host(case["grids"], anchors, nc)
        rb, rc, rp = (np.ascontiguousarray(a, np.float32) for a in (rb, rc, rp))
        B, N = rc.shape[:2]
        cls = np.empty((B, N), np.int64)
        scores = np.empty((B, N), np.float32)
        O.lib().y3o_scores(rc.reshape(-1), rp, B * N, nc, cls.reshape(-1), scores.reshape(-1))
        out = (rb, rc.reshape(B, N), rp, cls, scores)
        for a in out:
            a.setflags(write=False)
        _ref_cache[key] = out
    return _ref_cache[key]


def check_claims(case, boxes, conf, probs, cls, scores):
    """What a case claims, asserted exactly on one implementation's outputs (the CPU reference in the host tier, the device's in
    the GPU tier): conf [B,N], probs [B,N,nc], cls [B,N], scores [B,N], boxes [B,N,4], all NumPy."""
    name = case["name"]
    one, zero = np.float32(1.0), np.float32(0.0)
    if case["cls"] is not None:
        bad = np.argwhere(cls != case["cls"])
        assert bad.size == 0, (name, "class index", bad[:5].tolist(), cls[tuple(bad[0])], case["cls"][tuple(bad[0])])
    assert (probs[case["prob_one"]] == one).all() and (probs[case["prob_zero"]] == zero).all(), (name, "saturated probabilities")
    assert not np.signbit(probs[case["prob_zero"]]).any(), (name, "-0.0 probability")
    assert (conf[case["conf_one"]] == one).all() and (conf[case["conf_zero"]] == zero).all(), (name, "saturated objectness")
    assert np.array_equal(scores[case["score_conf"]], conf[case["score_conf"]]), (name, "score != objectness")
    assert (scores[case["score_zero"]] == zero).all(), (name, "score != 0")
    assert not np.isnan(boxes).any() and not np.isnan(scores).any() and not np.isnan(probs).any() and not np.isnan(conf).any(), (name, "NaN")
    assert np.array_equal(np.isposinf(boxes), case["box_inf"] == 1) and np.array_equal(np.isneginf(boxes), case["box_inf"] == -1), (name, "inf")
    w0, h0 = case["wh_zero"][..., 0], case["wh_zero"][..., 1]
    assert np.array_equal(boxes[..., 0][w0], boxes[..., 2][w0]) and np.array_equal(boxes[..., 1][h0], boxes[..., 3][h0]), (name, "zero size")
