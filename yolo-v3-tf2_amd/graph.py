"""Model description -> flat conv program.

Reads the model YAML schema of the reference's graph builder
(reference: core/parse_model.py:216-314 `create_sub_model_inputs`,
`create_sub_model_layers`, `build_model`) and produces

  * a node list with the reference's layer semantics (conv / maxpool / shortcut / route /
    upsample / yolo, reference: core/parse_model.py:13-56,59-75,78-99,102-160,209-213);
  * a *lowered* program for the HIP runtime in which BatchNorm, LeakyReLU, the
    shortcut add and the nearest-upsample + channel-concat feeding a 1x1 conv
    are folded into the conv launches.  A max-pool is never folded: it
    is an op of its own between two conv launches.

No arithmetic happens here; this is host logic only and runs without a GPU.
"""
from __future__ import annotations

import ast
import numbers
import operator
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import yaml

# ----------------------------------------------------------------------------
# tiny arithmetic evaluator (the reference calls eval() on `filters` strings,
# core/parse_model.py:258-259; we accept the same expressions without eval)
# ----------------------------------------------------------------------------
_BINOPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul,
           ast.FloorDiv: operator.floordiv}


def eval_int_expr(expr, names: Dict[str, int]) -> int:
    if isinstance(expr, int):
        return expr

    def ev(n):
        if isinstance(n, ast.Expression):
            return ev(n.body)
        if isinstance(n, ast.Constant) and isinstance(n.value, int):
            return n.value
        if isinstance(n, ast.Name) and n.id in names:
            return names[n.id]
        if isinstance(n, ast.BinOp) and type(n.op) in _BINOPS:
            return _BINOPS[type(n.op)](ev(n.left), ev(n.right))
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, ast.USub):
            return -ev(n.operand)
        raise ValueError(f"unsupported expression in model config: {expr!r}")

    return int(ev(ast.parse(str(expr), mode="eval")))


# ----------------------------------------------------------------------------
# node-level graph (reference semantics, nothing fused)
# ----------------------------------------------------------------------------
@dataclass
class Tensor:
    id: int
    channels: int
    div: int            # spatial size = image_size // div
    producer: str = ""  # debugging aid
    yolo: bool = False  # viewed as [B,g,g,3,5+nc]


@dataclass
class Node:
    kind: str                       # conv | maxpool | add | upsample | concat | yolo
    inputs: List[int]
    output: int
    # conv attributes (maxpool: size 2, stride 1 or 2)
    size: int = 0
    stride: int = 1
    filters: int = 0
    bn: bool = False
    leaky: bool = False
    conv_index: int = -1            # creation order == Darknet weight order
    sub_model: str = ""


@dataclass
class ConvOp:
    """One launch of the fused conv kernel.  cin / c0 / cout are the widths the launch sees: the stored widths of its tensors
    (Program.stored), which exceed the node's real widths where the lowering pads channels."""
    conv_index: int
    size: int
    stride: int
    cin: int
    cout: int
    bn: bool
    leaky: bool
    src0: int                       # tensor id holding input channels [0, c0)
    src0_upsample: bool             # src0 is read through a nearest x2 up-sampling
    c0: int
    src1: int                       # -1 or tensor id holding channels [c0, cin)
    residual: int                   # -1 or tensor id added after the activation
    dst: int
    in_div: int                     # input spatial divisor (after up-sampling)
    out_div: int


@dataclass
class AuxOp:
    kind: str                       # add | upsample | concat | maxpool_s2 | maxpool_s1
    inputs: List[int]
    dst: int


@dataclass
class Program:
    tensors: List[Tensor]
    nodes: List[Node]
    ops: list                       # ConvOp | AuxOp in execution order
    input_tensor: int
    outputs: List[int]              # head outputs in model order, coarsest grid first: three (YOLOv3) or two (YOLOv3-tiny)
    nclasses: int
    conv_nodes: List[Node] = field(default_factory=list)
    # per tensor id: the channel count the device stores (_lower).  tensors[t].channels everywhere except behind a conv whose
    # output width is no multiple of 32 and feeds another conv, directly or through pools: that tensor and the pooled ones are
    # stored padded to the next multiple of 32, the pad channels exact zeros (weights.pad_weights).
    stored: List[int] = field(default_factory=list)
    model_config_file: Optional[str] = None   # the model.yaml this program was read from (load_program)

    def conv_ops(self) -> List[ConvOp]:
        return [o for o in self.ops if isinstance(o, ConvOp)]

    def grid_sizes(self, image_size):
        """Per head (coarsest first): g = S // div for an int S; (gh, gw) = (H // div, W // div) for an (H, W) pair."""
        divs = [self.tensors[o].div for o in self.outputs]
        if isinstance(image_size, numbers.Integral):
            return [int(image_size) // d for d in divs]
        h, w = (int(v) for v in image_size)
        return [(h // d, w // d) for d in divs]

    def flops_per_image(self, image_size, backbone_only: bool = False) -> float:
        """2*MAC over the convolutions (SURVEY.md 8d algorithmic work); image_size: an int S or an (H, W) pair."""
        h, w = (image_size, image_size) if isinstance(image_size, numbers.Integral) else image_size
        tot = 0.0
        for n in self.conv_nodes:
            if backbone_only and n.sub_model != "backbone":
                continue
            t_in = self.tensors[n.inputs[0]]
            t_out = self.tensors[n.output]
            tot += 2.0 * n.size * n.size * t_in.channels * n.filters * (h // t_out.div) * (w // t_out.div)
        return tot

    def n_params(self) -> int:
        tot = 0
        for n in self.conv_nodes:
            cin = self.tensors[n.inputs[0]].channels
            tot += n.size * n.size * cin * n.filters + (4 * n.filters if n.bn else n.filters)
        return tot


class _Builder:
    def __init__(self, nclasses: int, config_root: Optional[str]):
        self.tensors: List[Tensor] = []
        self.nodes: List[Node] = []
        self.nclasses = nclasses
        self.nconv = 0
        self.root = config_root

    def new_tensor(self, channels, div, producer="", yolo=False) -> int:
        t = Tensor(len(self.tensors), channels, div, producer, yolo)
        self.tensors.append(t)
        return t.id

    # reference: core/parse_model.py:13-56
    def conv(self, x, conf, sub):
        stride, filters, size = int(conf["stride"]), int(conf["filters"]), int(conf["size"])
        act = conf["activation"]
        assert act in ("linear", "leaky"), "Invalid activation: {}".format(act)
        tin = self.tensors[x]
        if stride > 1 and (stride != 2 or size != 3):
            raise ValueError("only the 3x3/2 down-sampling conv of the reference is supported")
        out = self.new_tensor(filters, tin.div * stride, f"{sub}.conv{self.nconv}")
        self.nodes.append(Node("conv", [x], out, size=size, stride=stride, filters=filters,
                               bn="batch_normalize" in conf, leaky=(act == "leaky"),
                               conv_index=self.nconv, sub_model=sub))
        self.nconv += 1
        return out

    # reference: core/parse_model.py:78-99 (MaxPooling2D(size, stride, 'same'))
    def maxpool(self, x, conf, sub):
        who = f"{sub}.maxpool (layer {len(self.nodes)})"
        try:
            size, stride = [int(v) for v in conf["size_xy"]], [int(v) for v in conf["stride_xy"]]
        except (KeyError, TypeError, ValueError):
            raise ValueError(f"{who}: needs size_xy and stride_xy, two ints each") from None
        if len(size) != 2 or len(stride) != 2 or size[0] != size[1] or stride[0] != stride[1]:
            raise ValueError(f"{who}: size_xy {size} / stride_xy {stride}: only equal x and y are supported")
        if size[0] != 2 or stride[0] not in (1, 2):
            raise ValueError(f"{who}: size {size[0]} stride {stride[0]}: only the 2x2 pools of stride 1 and 2 are supported")
        if conf.get("padding", "valid") != "same":
            raise ValueError(f"{who}: padding {conf.get('padding', 'valid')!r}: only 'same' is supported")
        t = self.tensors[x]
        if stride[0] == 2 and t.div >= 32:
            raise ValueError(f"{who}: a stride-2 pool on a 1/{t.div} tensor: its extent is odd for image sizes that are "
                             f"multiples of 32 only")
        out = self.new_tensor(t.channels, t.div * stride[0], f"{sub}.maxpool")
        self.nodes.append(Node("maxpool", [x], out, size=2, stride=stride[0], sub_model=sub))
        return out

    # reference: core/parse_model.py:143-160
    def shortcut(self, x, conf, layers, sub):
        assert conf["activation"] == "linear", "Invalid activation: {}".format(conf["activation"])
        frm = layers[int(conf["from"])]
        a, b = self.tensors[frm], self.tensors[x]
        if (a.channels, a.div) != (b.channels, b.div):
            raise ValueError("shortcut operands differ in shape")
        out = self.new_tensor(a.channels, a.div, f"{sub}.add")
        self.nodes.append(Node("add", [frm, x], out, sub_model=sub))
        return out

    # reference: core/parse_model.py:102-140
    def route(self, conf, inputs_entry, layers, sub):
        sel = []
        if "layers" in conf["source"]:
            sel = [layers[int(i)] for i in conf["source"]["layers"]]
        if "inputs" in conf["source"]:
            if isinstance(inputs_entry, list):
                sel += [inputs_entry[i] for i in conf["source"]["inputs"]]
            else:
                sel += [inputs_entry]
        if len(sel) == 1:
            return sel[0]
        if len(sel) == 2:
            a, b = self.tensors[sel[0]], self.tensors[sel[1]]
            if a.div != b.div:
                raise ValueError("route operands differ in spatial size")
            out = self.new_tensor(a.channels + b.channels, a.div, f"{sub}.concat")
            self.nodes.append(Node("concat", list(sel), out, sub_model=sub))
            return out
        raise ValueError("Invalid number of layers: {}".format(len(sel)))

    # reference: core/parse_model.py:59-75
    def upsample(self, x, conf, sub):
        s = int(conf["stride"])
        if s != 2:
            raise ValueError("only x2 up-sampling is supported")
        t = self.tensors[x]
        if t.div % 2:
            raise ValueError("cannot up-sample past the input resolution")
        out = self.new_tensor(t.channels, t.div // 2, f"{sub}.up")
        self.nodes.append(Node("upsample", [x], out, sub_model=sub))
        return out

    # reference: core/parse_model.py:209-213 (Reshape to [g,g,3,5+nc]; a view)
    def yolo(self, x, sub):
        t = self.tensors[x]
        if t.channels != 3 * (5 + self.nclasses):
            raise ValueError("yolo layer input must have 3*(5+nclasses) channels")
        out = self.new_tensor(t.channels, t.div, f"{sub}.yolo", yolo=True)
        self.nodes.append(Node("yolo", [x], out, sub_model=sub))
        return out

    # reference: core/parse_model.py:248-278
    def sub_model_layers(self, layers_config, inputs, sub):
        x = inputs if not isinstance(inputs, list) else None
        layers: List[int] = []
        for conf in layers_config:
            conf = dict(conf)
            kind = conf["type"]
            if kind == "convolutional":
                conf["filters"] = eval_int_expr(conf["filters"], {"nclasses": self.nclasses})
                x = self.conv(x, conf, sub)
            elif kind == "shortcut":
                x = self.shortcut(x, conf, layers, sub)
            elif kind == "yolo":
                x = self.yolo(x, sub)
            elif kind == "route":
                x = self.route(conf, inputs, layers, sub)
            elif kind == "upsample":
                x = self.upsample(x, conf, sub)
            elif kind == "maxpool":
                x = self.maxpool(x, conf, sub)
            else:
                raise ValueError("{} not recognized as layer_conf type".format(kind))
            layers.append(x)
        return layers


def _resolve(path, root):
    if os.path.isabs(path) or os.path.exists(path) or root is None:
        return path
    return os.path.join(root, path)


def build_program(sub_models_configs: Sequence[dict], output_stage: str = "head", nclasses: int = 80,
                  config_root: Optional[str] = None, in_channels: int = 3) -> Program:
    """reference: core/parse_model.py:279-314 (build_model)."""
    b = _Builder(nclasses, config_root)
    model_input = b.new_tensor(in_channels, 1, "input")
    subs = []  # [{'name':..., 'outputs': [tensor ids]}]
    for cfg in sub_models_configs:
        name = cfg["name"]
        inputs_config = cfg.get("inputs")
        if inputs_config:
            if "shape" in inputs_config:
                raise ValueError("explicit input shapes are not supported; the model input is [B,S,S,3]")
            data_inputs = []
            for src in inputs_config["source"]:
                found = [s for s in subs if s["name"] == src["name"]]
                if not found:
                    raise Exception(f'Error: sub-model {src["name"]} not found')
                outs = found[0]["outputs"]
                # Keras hands back a bare tensor for single-output sub-models, so the reference
                # honours entry_index only for multi-output producers (core/parse_model.py:233-241)
                idx = src.get("entry_index", 0) if len(outs) > 1 else 0
                data_inputs.append(outs[idx])
            sub_inputs = data_inputs[0] if len(data_inputs) == 1 else data_inputs
        else:
            sub_inputs = model_input
        with open(_resolve(cfg["layers_config_file"], config_root), "r") as f:
            layers_config = yaml.safe_load(f)["layers_config"]
        layers = b.sub_model_layers(layers_config, sub_inputs, name)
        subs.append({"name": name, "outputs": [layers[int(i)] for i in cfg["outputs_layers"]]})
    outputs = []
    for s in subs:
        if output_stage in s["name"]:
            outputs += s["outputs"]
    prog = Program(b.tensors, b.nodes, [], model_input, outputs, nclasses)
    prog.conv_nodes = [n for n in b.nodes if n.kind == "conv"]
    _lower(prog)
    return prog


def find_config_root(model_config_file: str, sub_models_configs) -> Optional[str]:
    """Paths inside model.yaml are relative to the directory the reference is run from; when the process runs
    elsewhere, walk up from the model file until they resolve."""
    probe = sub_models_configs[0]["layers_config_file"]
    if os.path.isabs(probe) or os.path.exists(probe):
        return None
    d = os.path.dirname(os.path.abspath(model_config_file))
    while d != os.path.dirname(d):
        if os.path.exists(os.path.join(d, probe)):
            return d
        d = os.path.dirname(d)
    return None


def load_program(model_config_file: str, nclasses: int = 80) -> Program:
    with open(model_config_file, "r") as f:
        cfg = yaml.safe_load(f)
    root = find_config_root(model_config_file, cfg["sub_models_configs"])
    prog = build_program(cfg["sub_models_configs"], cfg.get("output_stage", "head"), nclasses, root)
    prog.model_config_file = os.path.abspath(model_config_file)
    return prog


# ----------------------------------------------------------------------------
# lowering: fold add / upsample / concat into conv launches where legal
# ----------------------------------------------------------------------------
def _lower(p: Program):
    consumers: Dict[int, List[Node]] = {}
    for n in p.nodes:
        for i in n.inputs:
            consumers.setdefault(i, []).append(n)
    producer = {n.output: n for n in p.nodes}
    external = set(p.outputs)
    folded = set()          # node outputs that never materialise
    alias: Dict[int, int] = {}

    def real(t):
        while t in alias:
            t = alias[t]
        return t

    # Channel padding: a conv output of a width that is no multiple of 32 is stored padded when everything that reads it, directly
    # or through pools only, is a conv (the device's convs take Cin % 32 == 0); the pools carry the padded width.
    stored = [t.channels for t in p.tensors]
    for n in p.nodes:
        if n.kind != "conv" or n.filters % 32 == 0:
            continue
        chain, todo, convs = [n.output], [n.output], 0
        while todo:
            t = todo.pop()
            if t in external:
                convs = -1
                break
            for c in consumers.get(t, []):
                if c.kind == "maxpool":
                    chain.append(c.output)
                    todo.append(c.output)
                elif c.kind == "conv" and convs >= 0:
                    convs += 1
                else:
                    convs = -1
            if convs < 0:
                break
        if convs > 0:
            for t in chain:
                stored[t] = (n.filters + 31) // 32 * 32
    p.stored = stored

    ops = []
    for n in p.nodes:
        if n.kind == "yolo":
            alias[n.output] = n.inputs[0]       # pure view
            continue
        if n.kind == "conv":
            src = n.inputs[0]
            tin = p.tensors[src]
            op = ConvOp(n.conv_index, n.size, n.stride, stored[src], stored[n.output], n.bn, n.leaky,
                        src0=real(src), src0_upsample=False, c0=stored[src], src1=-1, residual=-1,
                        dst=n.output, in_div=tin.div, out_div=p.tensors[n.output].div)
            pn = producer.get(src)
            # K6: [upsample(a), b] concat -> 1x1 conv; read both sources in the conv's A-gather
            if (pn is not None and pn.kind == "concat" and n.size == 1 and src not in external
                    and len(consumers.get(src, [])) == 1):
                a, bsrc = pn.inputs
                pa = producer.get(a)
                ca = p.tensors[a].channels
                if ca % 32 == 0:
                    op.c0, op.src1 = ca, real(bsrc)
                    if (pa is not None and pa.kind == "upsample" and a not in external
                            and len(consumers.get(a, [])) == 1):
                        op.src0, op.src0_upsample = real(pa.inputs[0]), True
                        folded.add(a)
                    else:
                        op.src0 = real(a)
                    folded.add(src)
            # K5: conv -> add(from, conv) with the conv feeding nothing else
            cons = consumers.get(n.output, [])
            if (len(cons) == 1 and cons[0].kind == "add" and n.output not in external
                    and cons[0].inputs[1] == n.output and cons[0].inputs[0] != n.output):
                op.residual = real(cons[0].inputs[0])
                op.dst = cons[0].output
                folded.add(cons[0].output)
                alias[n.output] = cons[0].output
            ops.append(op)
        elif n.kind in ("add", "upsample", "concat"):
            if n.output in folded:
                continue
            ops.append(AuxOp(n.kind, [real(i) for i in n.inputs], n.output))
        elif n.kind == "maxpool":               # never folded
            ops.append(AuxOp(f"maxpool_s{n.stride}", [real(n.inputs[0])], n.output))
    # drop aux producers that were folded away before being visited (upsample/concat precede the conv)
    ops = [o for o in ops if not (isinstance(o, AuxOp) and o.dst in folded)]
    p.ops = ops
    p.outputs = [real(o) for o in p.outputs]


def tiny_stem_applicable(p: Program) -> bool:
    """Does the lowered program start with the stem of YOLOv3-tiny, which Net.set_tiny_stem_fusion runs as one kernel (include/y3.h,
    y3_net_set_tiny_stem_fusion)?  Op 0 the first-layer conv 3x3 / 1, 3 -> 16 (stored 32) on the input, op 1 a max-pool 2x2 / 2 on it, op 2
    a 3x3 / 1 conv 16 (stored 32) -> 32 with one source and no shortcut, op 3 a max-pool 2x2 / 2 on it; each of the first three outputs
    has exactly one reader and none of the four is a net output.  The device decides the same from the stored widths and conv0's weights."""
    ops = p.ops
    if len(ops) < 5 or not (isinstance(ops[0], ConvOp) and isinstance(ops[1], AuxOp) and isinstance(ops[2], ConvOp) and isinstance(ops[3], AuxOp)):
        return False
    c0, p0, c1, p1 = ops[:4]
    stored = p.stored or [t.channels for t in p.tensors]
    if not (c0.size == 3 and c0.stride == 1 and c0.cin == 3 and c0.src0 == p.input_tensor and c0.src1 < 0 and c0.residual < 0
            and p.tensors[c0.dst].channels == 16 and stored[c0.dst] == 32):
        return False
    if not (p0.kind == "maxpool_s2" and p0.inputs == [c0.dst] and p1.kind == "maxpool_s2" and p1.inputs == [c1.dst]):
        return False
    if not (c1.size == 3 and c1.stride == 1 and c1.src0 == p0.dst and c1.src1 < 0 and c1.residual < 0 and not c1.src0_upsample
            and p.tensors[p0.dst].channels == 16 and c1.cin == 32 and c1.cout == 32 and p.tensors[c1.dst].channels == 32):
        return False
    if any(t in p.outputs for t in (c0.dst, p0.dst, c1.dst, p1.dst)):
        return False
    for t in (c0.dst, p0.dst, c1.dst):
        readers = sum((o.src0 == t) + (o.src1 == t) + (o.residual == t) if isinstance(o, ConvOp) else o.inputs.count(t) for o in ops)
        if readers != 1:
            return False
    return True
