"""Canonical, pointer-free text dump of launch plans (CPU only, nothing is launched): the instrument that shows a change to
the plan builder (mi355/graph.py) left every launch table as it was.

    python scripts/plan_dump.py OUT_DIR [--tree REPO_ROOT] [--jobs N] [--only SUBSTRING]

writes one file per configuration (model x shape x dtype x mode, block-level plans, and every builder switch set to 0 on its
own — the switches are read at import, so each runs in a fresh process).  ``--tree`` imports the package of ANOTHER checkout
(with its library built), so that

    python scripts/plan_dump.py /tmp/a --tree /path/to/parent && python scripts/plan_dump.py /tmp/b && diff -r /tmp/a /tmp/b

compares two commits.  Only the public Plan / Launch / T / V / GRef / Ws surface is used.

One line per launch of pre / fwd / bwd: name, tag, flops, bytes, side, cus, then every argument.  Activations are written as
their buffer's number in order of first appearance, element offset, N x H x W x C and row pitch; parameters and module buffers
by name; parameter gradients as name + byte offset inside the parameter's slot; workspaces by kind (+ byte offset); floats as
their repr; the batched weight-pack table row by row with its pointers mapped through the same numbering (a pointer to
nothing known is an error)."""
import argparse
import os
import subprocess
import sys

SWITCHES = ("MI355_FUSE_POOL", "MI355_FUSE_POOL_BWD", "MI355_FUSE_GATE_BWD", "MI355_FUSE_HEAD", "MI355_BN_ACT_WINDOWS",
            "MI355_BN_ACT_WINDOWS_RES", "MI355_FUSE_RESIDUAL", "MI355_DEFER_POST", "MI355_SIDE_COLSUM", "MI355_WGRAD_MULTI",
            "MI355_TAIL_ON_MAIN", "MI355_STEM_IM2COL")
S64, S32 = (2, 3, 64, 64), (2, 3, 32, 32)
MODELS = {      # name -> input shapes
    "AttentionUNet": [S64, (1, 3, 48, 48), (1, 3, 80, 80)],      # 48: odd 3 x 3 bottom level; 80: W = 40, no pool2 backward
    "R2AttU_Net": [(1, 3, 32, 32), S32], "R2U_Net": [(1, 3, 32, 32), S32],
    "ResNetUnet_frozen": [S64, (1, 3, 64, 64)], "ResNetUnet_unfrozen": [S64, (1, 3, 64, 64)],
    "ResNet18": [S64], "ResNet50": [S64], "resnet18_tv": [S64], "VGG16": [S32], "VGG16_BN": [S32],
    "ResNet18_head_only": [S64],                                  # stage 1 of the classification protocol
}
CLASSIFIERS = ("ResNet18", "ResNet50", "resnet18_tv", "VGG16", "VGG16_BN", "ResNet18_head_only")
SWITCHED = {"AttentionUNet": S64, "R2AttU_Net": (1, 3, 32, 32), "ResNet18": S64}
BLOCKS = {      # block-level plans (want_input_grad + tensor_output): tag -> (constructor args, input shapes)
    "basic_block": ((32, 64), [(2, 32, 12, 12)]), "UpConv": ((64, 32), [(2, 64, 6, 6)]),
    "AttentionGate": ((64, 64, 32), [(2, 64, 8, 8), (2, 64, 8, 8)]), "RRCNN_block": ((32, 64, 2), [(2, 32, 8, 8)]),
    "BasicBlock_s2": ((32, 64, 2), [(2, 32, 8, 8)]), "DecoderBlock": ((96, 32), [(2, 64, 8, 8), (2, 32, 8, 8)]),
    **{f"Recurrent_block_t{t}": ((32, 32, t), [(2, 32, 8, 8)]) for t in (2, 5, 7, 10)},
}


def configs():
    """[(file stem, switch set to 0 or None, model or block tag, shape, dtype name, mode)]"""
    out = []
    for dt in ("fp32", "bf16"):
        for name, shapes in MODELS.items():
            for shape in shapes:
                for mode in ("train", "eval") + (("explain",) if name in CLASSIFIERS else ()):
                    out.append((f"{name}_{'x'.join(map(str, shape))}_{dt}_{mode}", None, name, shape, dt, mode))
        for tag in BLOCKS:
            out.append((f"block_{tag}_{dt}_train", None, "block:" + tag, None, dt, "train"))
    for sw in SWITCHES:
        for name, shape in SWITCHED.items():
            for mode in ("train", "eval"):
                out.append((f"{name}_{'x'.join(map(str, shape))}_bf16_{mode}_{sw}=0", sw, name, shape, "bf16", mode))
    return out


# ---- models -------------------------------------------------------------------------------------------------------------------
def make_model(name):
    if name.startswith("block:"):
        return make_block(name[6:])
    if name.startswith("ResNetUnet"):
        from models.segmentation_models.ResnetUnet import ResNetUnet
        return ResNetUnet(freeze=name.endswith("_frozen"))
    if name == "ResNet18_head_only":
        from models.classification_models.ResNet import ResNet18
        from utils.helpers import add_dropout_to_fc
        net = ResNet18(num_classes=1000)
        head = add_dropout_to_fc(net, p=0.5)
        for p in net.parameters():
            p.requires_grad = False
        for p in getattr(net, head).parameters():
            p.requires_grad = True
        return net
    if name in ("AttentionUNet", "R2AttU_Net", "R2U_Net"):
        mod = __import__("models.segmentation_models." + name, fromlist=[name])
        return getattr(mod, name)()
    from models.classification_models import ResNet, TorchvisionResNet, VGG
    return {"ResNet18": ResNet.ResNet18, "ResNet50": ResNet.ResNet50, "resnet18_tv": TorchvisionResNet.resnet18,
            "VGG16": VGG.VGG16, "VGG16_BN": VGG.VGG16_BN}[name](3)


def make_block(tag):
    """One building block as a network of its own, the way tests/test_gpu_blocks.py wraps them."""
    from mi355.engine import Net
    from models.segmentation_models import _blocks as B
    args, shapes = BLOCKS[tag]
    if tag == "basic_block":
        blk, low = B.conv_bn_relu_x2(*args), lambda g, b, xs: g.seq(b, xs[0])
    elif tag == "UpConv":
        blk, low = B.UpConv(*args), lambda g, b, xs: g.seq(b.up, xs[0])
    elif tag == "AttentionGate":
        blk, low = B.AttentionGate(*args), lambda g, b, xs: g.gate(b, g=xs[0], x=xs[1])
    elif tag.startswith("Recurrent_block"):
        blk, low = B.Recurrent_block(args[0], args[1], t=args[2]), lambda g, b, xs: b.lower(g, xs[0])
    elif tag == "RRCNN_block":
        blk, low = B.RRCNN_block(args[0], args[1], t=args[2]), lambda g, b, xs: b.lower(g, xs[0])
    elif tag == "DecoderBlock":
        from models.segmentation_models.ResnetUnet import DecoderBlock
        blk, low = DecoderBlock(*args), lambda g, b, xs: b.lower(g, g.maxpool(xs[0], 2, 2, 0), xs[1])
    else:
        from models.classification_models.ResNet import BasicBlock
        blk, low = BasicBlock(args[0], args[1], stride=args[2]), lambda g, b, xs: b.lower(g, xs[0])
    chans = [s[1] for s in shapes]

    class BlockNet(Net):
        def __init__(self):
            super().__init__()
            self.block = blk

        def build(self, g, x):
            g.want_input_grad(x)
            xs, o = [], 0
            for c in chans:
                xs.append(g.slice_channels(x, o, c) if len(chans) > 1 else x)
                o += c
            g.tensor_output(low(g, self.block, xs))

    net = BlockNet()
    net.dump_shape = (shapes[0][0], sum(chans), shapes[0][2], shapes[0][3])
    return net


def build_plan(name, shape, dt, mode):
    import torch
    net = make_model(name).train(mode == "train")
    net.engine.flatten()
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[dt]
    train = mode == "train"
    return net, net.engine.plan_for(shape or net.dump_shape, train, train, dtype, explain=(mode == "explain"))


# ---- the dump ------------------------------------------------------------------------------------------------------------------
class Dumper:
    def __init__(self, net, plan):
        import torch
        from mi355 import graph
        self.torch, self.g, self.plan, self.eng = torch, graph, plan, plan.engine
        self.names = {}
        for k, t in list(net.named_parameters()) + list(net.named_buffers()):
            self.names.setdefault(t.data_ptr(), k)
        self.ws = {t.data_ptr(): k for k, t in plan.ws.items()}
        self.kept = {t.data_ptr(): t for t in plan.keep}
        self.numbers = {}
        self.lines = []

    def buf(self, t):
        p = t.data_ptr()
        if p in self.names:
            return self.names[p]
        if p in self.ws:
            return "ws:" + self.ws[p]
        n = self.numbers.setdefault(p, len(self.numbers))
        return f"b{n}<{str(t.dtype).replace('torch.', '')}*{t.numel()}>"

    def ptr(self, p):
        """A raw device pointer (weight-pack table): what it points to, by the numbering of the launch arguments."""
        if p == 0:
            return "-"
        if p in self.names:
            return self.names[p]
        if p not in self.kept:
            raise ValueError(f"pointer {p:#x} in a weight-pack table points to no parameter, module buffer or plan buffer")
        return self.buf(self.kept[p])

    def fmt(self, a):
        g = self.g
        if a is None:
            return "-"
        if isinstance(a, g.T):
            return f"{self.buf(a.buf)}+{a.off}:{a.N}x{a.H}x{a.W}x{a.C}/{a.ld}"
        if isinstance(a, g.V):
            return f"{self.buf(a.buf)}:{a.B}x{a.F}"
        if isinstance(a, g.GRef):
            return f"grad({self.names[a.param.data_ptr()]})+{a.off - self.eng.grad_ref(a.param).off}"
        if isinstance(a, g.Ws):
            return "ws:" + a.kind
        if isinstance(a, self.torch.Tensor):
            return self.buf(a)
        if isinstance(a, tuple) and len(a) == 2 and isinstance(a[0], self.torch.Tensor) and isinstance(a[1], int):      # (tensor, byte offset)
            return f"{self.buf(a[0])}@{a[1]}"
        if isinstance(a, (tuple, list)):
            return "(" + ",".join(self.fmt(v) for v in a) + ")"
        if isinstance(a, bool):
            return str(int(a))
        if isinstance(a, float):
            return repr(a)
        if isinstance(a, (int, str)):
            return str(a)
        raise TypeError(f"no canonical form for a launch argument of type {type(a).__name__}")

    def launch(self, where, i, l):
        if not isinstance(l, self.g.Launch):
            raise TypeError(f"{where}[{i}] is a {type(l).__name__}, not a Launch")
        self.lines.append(f"{where}[{i}] {l.name} tag={l.tag or '-'} flops={l.flops} bytes={l.bytes} side={int(l.side)} cus={l.cus!r} | "
                          + " ".join(self.fmt(a) for a in l.args))
        if l.name == "mi355_pack_conv_weights_batched":
            for r, row in enumerate(l.args[0].tolist()):
                w, wf, wb, co, ci, cip, taps, tr, sc = row
                self.lines.append(f"    pack[{r}] w={self.ptr(w)} wf={self.ptr(wf)} wb={self.ptr(wb)} co={co} ci={ci} cip={cip} taps={taps} "
                                  f"transposed={tr} scale={self.ptr(sc)}")

    def text(self):
        plan = self.plan
        for where in ("pre", "fwd", "bwd"):
            for i, l in enumerate(getattr(plan, where)):
                self.launch(where, i, l)
        if plan.static_pack is not None:
            self.launch("static_pack", 0, plan.static_pack)
        name = lambda p: self.names[p.data_ptr()]
        by_id = {id(p): p for p in self.eng.params}
        out = self.lines
        out.append("static_params " + " ".join(name(p) for p in plan.static_params))
        out.append("ws " + " ".join(f"{k}={plan.ws[k].numel()}" for k in sorted(plan.ws)))
        out.append(f"keep_bytes {sum(t.numel() * t.element_size() for t in plan.keep)}")
        out.append("grad_params " + " ".join(name(p) for p in plan.grad_params))
        out.append("zero_grad_params " + " ".join(name(p) for p in plan.zero_grad_params))
        out.append("last_write " + " ".join(f"{name(by_id[i])}={n}" for i, n in plan.last_write.items()))
        for i, a in enumerate(plan.acts):
            out.append(f"acts[{i}] " + " ".join(self.fmt(v) for v in a))
        for k in ("input", "output", "dout", "input_grad", "cam", "cam_grad", "cam_target", "cam_lowres"):
            out.append(f"{k} {self.fmt(getattr(plan, k, None))}")
        return "\n".join(out) + "\n"


def dump_plan(net, plan):
    return Dumper(net, plan).text()


# ---- driver --------------------------------------------------------------------------------------------------------------------
def use_tree(root):
    root = os.path.abspath(root)
    for p in (os.path.join(root, "medical-image-segmentation-and-classification_amd"), root):
        if p not in sys.path:
            sys.path.insert(0, p)


def worker(out_dir, switch, model, only):
    import torch
    torch.set_num_threads(1)
    for stem, sw, name, shape, dt, mode in configs():
        if sw == switch and name == model and only in stem:
            net, plan = build_plan(name, shape, dt, mode)
            with open(os.path.join(out_dir, stem + ".txt"), "w") as f:
                f.write(dump_plan(net, plan))


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out_dir")
    ap.add_argument("--tree", default=here, help="repository root whose package is imported (its library must be built)")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", default="", help="only configurations whose file name contains this")
    ap.add_argument("--worker", nargs=2, metavar=("SWITCH", "MODEL"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        use_tree(a.tree)
        worker(a.out_dir, None if a.worker[0] == "-" else a.worker[0], a.worker[1], a.only)
        return
    os.makedirs(a.out_dir, exist_ok=True)
    groups = list(dict.fromkeys((sw, name) for stem, sw, name, *_ in configs() if a.only in stem))
    running, failed = [], 0
    while groups or running:
        while groups and len(running) < a.jobs:
            sw, name = groups.pop(0)
            env = dict(os.environ)
            for s in SWITCHES:
                env.pop(s, None)
            if sw:
                env[sw] = "0"
            running.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), a.out_dir, "--tree", a.tree, "--only", a.only,
                                             "--worker", sw or "-", name], env=env))
        failed += running.pop(0).wait() != 0
    files = sorted(f for f in os.listdir(a.out_dir) if f.endswith(".txt"))
    lines = sum(sum(1 for _ in open(os.path.join(a.out_dir, f))) for f in files)
    print(f"{len(files)} files, {lines} lines in {a.out_dir}" + (f"; {failed} worker(s) FAILED" if failed else ""))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
