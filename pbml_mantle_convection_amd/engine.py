"""Host-side executor of the Stokes-surrogate network on libmantle_hip (MI355X).

A network (Unet, ConvAE, or a single layer) is described as a small static graph of
conv / upsample nodes (`NetGraph`).  `Engine` resolves shapes for a given input size, owns
every device buffer (activations in the CB8 layout, GroupNorm statistics, filter banks,
gradient buffers, workspaces) and issues the C-ABI kernel calls for forward and backward
on the current HIP stream — so a whole training step can be captured into one HIP graph.

Reference call sites replaced: Unet.forward (pytorch_networks_convae.py:1985-2070),
ConvAE.forward (.ipynb_checkpoints/pycold-checkpoint.py:1094-1115), FluidLayer.forward
(:790-799) and the autograd backward of all of them.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import defaultdict
from dataclasses import dataclass
from enum import Enum
from typing import ClassVar, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L

# "mixed" = MC_MIX16: every tensor of the forward pass in f16 (11 significant bits: what the momentum residual's second
# differences need), every gradient tensor in bf16 (range), MFMA arithmetic with f32 accumulation.  (Round 2's form of the
# same idea -- bf16 everywhere, the full-resolution level of the forward pass as bf16 (hi, lo) pairs -- cost 1.1 ms per step
# more and was removed in round 3.)
DTYPES = {"fp32": (L.MC_F32, torch.float32), "f32": (L.MC_F32, torch.float32),
          "bf16": (L.MC_BF16, torch.bfloat16), "mixed": (L.MC_MIX16, torch.float16)}


# ------------------------------------------------------------------------------------------------
# static graph
# ------------------------------------------------------------------------------------------------
@dataclass
class ConvNode:
    name: str                  # state-dict prefix of the conv weight/bias ("conv.0.layers.0." ...)
    srcs: List[int]            # tensor ids (1 or 2: torch.cat order)
    out: int                   # tensor id of the activated output
    c_out: int
    k: int
    pad: int
    sym_h: int                 # 0 = plain nn.Conv2d
    post: int                  # L.POST_*
    gn_name: Optional[str]     # state-dict prefix of the GroupNorm affine or None
    groups: int
    pool: int = 1              # AvgPool factor applied to the activated output (1 = none)
    pooled: int = -1           # tensor id of the pooled output
    kind: str = "conv"
    learned: bool = False      # BoundaryLearnedConvolution2D ("learned padding"): nine valid banks + one shared bias,
    bc_x: int = 1              # name + {conv, conv_top_left, ...}.weight / name + learnable_bias; bc > 1 widens the
    bc_y: int = 1              # border strips so that the output grows (Unet's first layer, reference :1995)
    sym_v: int = 0             # y-mirrored filters / filters mirrored about both axes (SymmetricConv2d symmetry 'v' / 'hv';
    sym_hv: int = 0            # FluidLayer never sets them, reference :755-757)
    spectral: bool = False     # SpectralConv2d (reference :571-635): name + {weights1, weights2}, no bias; k = pad = sym = 0
    drop: float = 0.0          # nn.Dropout(p) after the activation (FluidLayer, reference :753, :798); training mode only
    layer: int = -1            # index among the graph's conv nodes in node order: the dropout mask's layer id


@dataclass
class UpNode:
    src: int
    out: int
    size: Optional[Tuple[int, int]] = None   # resolved at plan time (size of a named tensor)
    like: int = -1                           # take H, W of this tensor id ...
    scale: int = 0                           # ... or multiply by this integer scale factor
    kind: str = "up"


@dataclass
class PoolNode:                 # standalone nn.AvgPool2d(f, stride=f) (floor mode)
    src: int
    out: int
    f: int
    kind: str = "pool"


@dataclass
class CatNode:                  # torch.cat of several tensors along channels (any channel counts)
    srcs: List[int]
    out: int
    kind: str = "cat"


@dataclass
class NetGraph:
    c_in: int
    c_out: int
    channels: Dict[int, int]   # tensor id -> channel count
    nodes: list
    in_pad_w: int = 0          # F.pad(inputs, (3,3,0,0)) of the Unet
    crop_w: int = 0            # [..., 3:-3]
    subtract_mean: bool = False
    pad_mode: str = "zeros"
    act: str = "gelu"
    divisor: int = 1           # H, W must be divisible by this (ConvAE: 4**levels)
    input_grad: bool = False   # backward also produces the gradient w.r.t. the network input (single-layer graphs, tests)


def fluid_sym_h(c_o: int) -> int:
    """FluidLayer's mirrored filters: h = c_o/4 (c_o/2 if c_o <= 4), v = hv = 0 (reference pytorch_networks_convae.py:755-757)."""
    return int(c_o / 4) if c_o > 4 else int(c_o / 2)


def fluid_groups(c_o: int) -> int:
    """FluidLayer's GroupNorm groups (reference :788)."""
    return int(c_o / min(4, c_o))


class _Builder:
    """A graph under construction: the channel dict, the node list and the tensor-id counter (ids in call order of new())."""

    def __init__(self, c_i, f, use_symm, learned=False):
        self.ch: Dict[int, int] = {0: c_i}
        self.nodes = []
        self.f, self.use_symm, self.learned = f, use_symm, learned

    def new(self, c):
        tid = len(self.ch)
        self.ch[tid] = c
        return tid

    def conv(self, name, srcs, c_out, post, gn_name, groups, *, k=None, pad=None, symm=None, pool=1, out=None, **bc):
        """Appends a ConvNode: k x k (default f), 'same' padding unless `pad` says otherwise, output (then pooled output)
        allocated here unless the caller passes `out`.  symm: mirrored filters, where the network uses them at all; by default
        what the reference's heads do -- only as learned-padding layers (fixed padding: plain nn.Conv2d)."""
        k = self.f if k is None else k
        symm = self.learned if symm is None else symm
        node = ConvNode(name, list(srcs), self.new(c_out) if out is None else out, c_out, k, k // 2 if pad is None else pad,
                        fluid_sym_h(c_out) if (symm and self.use_symm) else 0, post, gn_name, groups, pool, learned=self.learned, **bc)
        if pool > 1:
            node.pooled = self.new(c_out)
        return self._append(node)

    def _append(self, node):
        node.layer = sum(1 for n in self.nodes if n.kind == "conv")
        self.nodes.append(node)
        return node

    def fluid(self, prefix, srcs, c_out, spectral=False, drop=0.0, **kw):
        """A FluidLayer: conv + GroupNorm + activation (+ dropout with rate `drop` in training mode); spectral: a
        SpectralFluidLayer (reference :638-699), whose GroupNorm has int(c_o / 4) groups and which has no dropout."""
        if spectral:
            if c_out < 4:
                raise ValueError(f"{prefix}: a spectral layer needs c_o >= 4 (GroupNorm has int(c_o / 4) groups), got {c_out}")
            node = ConvNode(prefix + "layers.0.", list(srcs), self.new(c_out), c_out, 0, 0, 0, L.POST_GN_ACT, prefix + "layers.1.",
                            int(c_out / 4), spectral=True, **kw)
            return self._append(node)
        node = self.conv(prefix + "layers.0.", srcs, c_out, L.POST_GN_ACT, prefix + "layers.1.", fluid_groups(c_out), symm=True, **kw)
        if drop:
            L.dropout_keep16(drop)                   # 0 <= p < 1, else ValueError
            if node.pool > 1:
                raise NotImplementedError(f"{prefix}: dropout on a layer that is pooled in its own launch is not built")
            node.drop = float(drop)
        return node


def unet_graph(levels, c_i, c_h, c_o, *, act, r_p, use_symm, repeats, f) -> NetGraph:
    """Layer wiring of Unet.__init__/forward (reference pytorch_networks_convae.py:1842-2024).  r_p = 'learned': every
    conv is a BoundaryLearnedConvolution2D node; the input is not padded — the first layer's bc_x = 4 strips grow the field
    by the same 3 + 3 columns (:1990-1997) — and the two-operand concats are materialised (CatNode).  With fixed padding a
    two-operand concat is the conv's two sources, unless its first operand does not fill whole channel blocks (c_h = 6, 12,
    ...: the two-source conv kernels need c_in0 % 8 == 0); that concat is materialised too."""
    if levels < 2:
        raise ValueError("Unet needs levels >= 2")
    learned = r_p == "learned"
    b = _Builder(c_i, f, use_symm, learned)
    ch, nodes = b.ch, b.nodes

    def one_src(srcs):
        if len(srcs) == 1 or (not learned and all(ch[i] % 8 == 0 for i in srcs[:-1])):
            return list(srcs)
        cat = b.new(sum(ch[i] for i in srcs))
        nodes.append(CatNode(list(srcs), cat))
        return [cat]

    def fluid(prefix, srcs, c_out, **kw):
        return b.fluid(prefix, one_src(srcs), c_out, **kw)

    feat = {}
    cur = 0
    for r in range(repeats):
        last = r == repeats - 1
        n = fluid(f"conv.{r}.", [cur], c_h, pool=2 if last else 1, bc_x=4 if (learned and r == 0) else 1)
        cur = n.out
    feat[0] = n
    c = c_h
    for l in range(1, levels):
        cur = feat[l - 1].pooled
        for r in range(repeats):
            last = r == repeats - 1
            n = fluid(f"convs.{l - 1}.{r}.", [cur], c, pool=2 if (last and l < levels - 1) else 1)
            cur = n.out
        feat[l] = n
        c *= 2
    c = int(c / 2)
    xu = feat[levels - 1].out
    for li, l in enumerate(range(levels - 2, 0, -1)):
        up = b.new(ch[xu])
        nodes.append(UpNode(xu, up, like=feat[l].out))
        srcs = [feat[l].out, up]
        for r in range(repeats):
            n = fluid(f"upconvs.{li}.{r}.", srcs, int(c / 2))
            srcs = [n.out]
        xu = n.out
        c = int(c / 2)
    up = b.new(ch[xu])
    nodes.append(UpNode(xu, up, like=feat[0].out))
    R = repeats

    def head(name, srcs, c_out, post, gn_name, groups):
        o = b.new(c_out)                     # (the head's output id precedes its concat's)
        return b.conv(name, one_src(srcs), c_out, post, gn_name, groups, out=o).out

    o = head(f"conv.{R}.", [up, feat[0].out], c, L.POST_GN_ACT, "gn.0.", int(c / 4))
    o2 = head(f"conv.{R + 1}.", [o], c, L.POST_ACT, None, 1)
    head(f"conv.{R + 2}.", [o2], c_o, L.POST_NONE, None, 1)
    return NetGraph(c_i, c_o, ch, nodes, in_pad_w=0 if learned else 3, crop_w=3, subtract_mean=True,
                    pad_mode="zeros" if learned else r_p, act=act, divisor=1)


def convae_graph(levels, c_i, c_h, c_o, *, act, r_p, use_symm, repeats, f, loss_type) -> NetGraph:
    """ConvAE.__init__ (reference .ipynb_checkpoints/pycold-checkpoint.py:1038-1092); returns the graph and
    keeps the ModuleList indices of the reference (pool / upsample modules consume an index)."""
    b = _Builder(c_i, f, use_symm)
    idx = [0]

    def fluid(src, c_out):
        idx[0] += 1
        return b.fluid(f"conv.{idx[0] - 1}.", [src], c_out)

    n = fluid(0, c_h)
    c = c_h
    for _ in range(levels):
        n.pool = 4
        n.pooled = b.new(n.c_out)
        idx[0] += 1                       # the AvgPool2d module
        cur = n.pooled
        cout = c * 4
        for r in range(repeats):
            n = fluid(cur, int(cout))
            cur = n.out
        c *= 4
    c = int(c / 4)
    cur = n.out
    for r in range(repeats):
        n = fluid(cur, c)
        cur = n.out
    for _ in range(levels, 0, -1):
        up = b.new(b.ch[cur])
        b.nodes.append(UpNode(cur, up, scale=4))
        idx[0] += 1                       # the Upsample module
        cur = up
        cout = int(c / 4)
        for r in range(repeats):
            n = fluid(cur, cout)
            cur = n.out
        c = int(c / 4)
    b.conv(f"conv.{idx[0]}.", [cur], int(c_o), L.POST_NONE, None, 1, k=3, pad=2 if loss_type == "curl" else 1)
    return NetGraph(c_i, int(c_o), b.ch, b.nodes, pad_mode=r_p, act=act, divisor=4 ** levels)


def _fluid_trunk(levels, c_i, c_h, *, r_p, use_symm, repeats, f, factor, spectral=False, drop_rate=0.0):
    """The multi-resolution trunk NewFluidNet and FluidNet share (reference pytorch_networks_convae.py:1315-1337 and
    :1642-1658): level l = the input feature map average-pooled l times, `repeats` FluidLayers, bicubic back to the input
    size; concat of the levels with the raw inputs.  The reference re-pools the feature map from scratch for every level; the
    values are identical to pooling the previous level once more, which is what the graph does.  Returns (builder, tensor id
    of the concat).  Any c_h with learned padding (the run list's configurations, pinned by the reference goldens); with fixed
    padding c_h must stay a multiple of 8.  spectral: every FluidLayer of the trunk is a SpectralFluidLayer (:1211-1254,
    :1535-1570); the heads stay what they are.  drop_rate: every (non-spectral) FluidLayer of the trunk ends in dropout
    (:1218, :1252); the heads have none."""
    learned = r_p == "learned"
    if c_h % 8 and not learned:
        raise NotImplementedError("the HIP path of NewFluidNet / FluidNet with fixed padding needs c_h to be a multiple of 8 "
                                  "(r_p='learned' takes any c_h)")
    b = _Builder(c_i, f, use_symm, learned)
    x_in = b.fluid("conv.0.", [0], c_h, spectral=spectral, drop=drop_rate).out
    pooled = x_in
    outs = []
    for l in range(levels):
        if l > 0:
            p = b.new(c_h)
            b.nodes.append(PoolNode(pooled, p, factor))
            pooled = p
        cur = pooled
        for r in range(repeats):
            cur = b.fluid(f"convs.{l}.{r}.", [cur], c_h, spectral=spectral, drop=drop_rate).out
        if l > 0:
            up = b.new(c_h)
            b.nodes.append(UpNode(cur, up, like=x_in))
            cur = up
        outs.append(cur)
    cat = b.new(c_h * levels + c_i)
    b.nodes.append(CatNode(outs + [0], cat))
    return b, cat


def _fluid_head(b, cat, c_h, c_o, *, act, r_p, **first) -> NetGraph:
    """conv.1 (+ gn.0 + act), conv.2 (+ act), conv.3 on the trunk's concat: 3 x 3 convs with fixed padding, k = f
    BoundaryLearnedConvolution2D layers with learned padding (reference :1296-1313).  first: what conv.1 alone takes."""
    k = b.f if b.learned else 3
    o = b.conv("conv.1.", [cat], c_h, L.POST_GN_ACT, "gn.0.", int(c_h / 4), k=k, **first).out
    o2 = b.conv("conv.2.", [o], c_h, L.POST_ACT, None, 1, k=k).out
    b.conv("conv.3.", [o2], c_o, L.POST_NONE, None, 1, k=k)
    c_i = b.ch[0]
    return NetGraph(c_i, c_o, b.ch, b.nodes, subtract_mean=True, pad_mode="zeros" if b.learned else r_p, act=act, divisor=1)


def newfluidnet_graph(levels, c_i, c_h, c_o, *, act, r_p, use_symm, repeats, f, factor=2, spectral=False, drop_rate=0.0) -> NetGraph:
    """Layer wiring of NewFluidNet.__init__/forward (reference pytorch_networks_convae.py:1215-1346): the shared trunk
    (_fluid_trunk), then the head (_fluid_head)."""
    b, cat = _fluid_trunk(levels, c_i, c_h, r_p=r_p, use_symm=use_symm, repeats=repeats, f=f, factor=factor, spectral=spectral,
                          drop_rate=drop_rate)
    return _fluid_head(b, cat, c_h, c_o, act=act, r_p=r_p)


def fluidnet_graph(levels, c_i, c_h, c_o, *, act, r_p, use_symm, repeats, f, factor=2, spectral=False, drop_rate=0.0) -> NetGraph:
    """Layer wiring of FluidNet.__init__/forward with loss_type 'curl' (reference pytorch_networks_convae.py:1581-1665): the
    trunk of NewFluidNet, then a head whose first conv grows the field by one pixel on every side, so that the output is
    (H + 2) x (W + 2) and the curl head's centred differences land on H x W (mc_curl_valid_*).  Learned padding: conv.1 is a
    k = f BoundaryLearnedConvolution2D called with bc_x = bc_y = 2 (:1660), conv.2 / conv.3 plain learned convs.  Fixed
    padding: conv.1 is the constructor's 3 x 3 conv with padding (2, 2), conv.2 / conv.3 3 x 3 with padding 1 (the reference's
    forward passes bc_x / bc_y to that nn.Conv2d and fails)."""
    b, cat = _fluid_trunk(levels, c_i, c_h, r_p=r_p, use_symm=use_symm, repeats=repeats, f=f, factor=factor, spectral=spectral,
                          drop_rate=drop_rate)
    return _fluid_head(b, cat, c_h, c_o, act=act, r_p=r_p, **(dict(bc_x=2, bc_y=2) if b.learned else dict(pad=2)))


def single_layer_graph(c_in, c_out, k, pad, pad_mode, sym_h, post, act, groups, gn: bool, learned: bool = False,
                       sym_v: int = 0, sym_hv: int = 0, bc_x: int = 1, bc_y: int = 1, input_grad: bool = False,
                       spectral: bool = False, drop_rate: float = 0.0) -> NetGraph:
    """One conv (+GN+act): SymmetricConv2d / FluidLayer / BoundaryLearnedConvolution2D (learned; bc_x, bc_y as in its forward)
    / SpectralConv2d / SpectralFluidLayer (spectral; k, pad, sym are ignored) used stand-alone.  input_grad (learned and
    spectral layers): backward leaves d(loss)/d(input) in Engine.input_grad_cb8().  drop_rate: dropout after the activation
    (FluidLayer; a spectral layer ignores it)."""
    if input_grad and not (learned or spectral):
        raise NotImplementedError("input_grad is implemented for learned-padding and spectral layers")
    ch = {0: c_in, 1: c_out}
    if spectral:
        node = ConvNode("layers.0." if gn else "", [0], 1, c_out, 0, 0, 0, post, "layers.1." if gn else None, groups, spectral=True,
                        layer=0)
        return NetGraph(c_in, c_out, ch, [node], pad_mode="zeros", act=act, input_grad=input_grad)
    node = ConvNode("layers.0." if gn else "", [0], 1, c_out, k, pad, sym_h, post, "layers.1." if gn else None, groups,
                    learned=learned, sym_v=sym_v, sym_hv=sym_hv, bc_x=bc_x, bc_y=bc_y, layer=0)
    if drop_rate:
        L.dropout_keep16(drop_rate)
        if post != L.POST_GN_ACT:
            raise NotImplementedError("dropout follows GroupNorm + activation (a FluidLayer)")
        node.drop = float(drop_rate)
    return NetGraph(c_in, c_out, ch, [node], pad_mode=pad_mode, act=act, input_grad=input_grad)


# learned padding (BoundaryLearnedConvolution2D): parameter order of the nine banks (the reference's sub-modules)
BANKS = ("conv", "conv_top_left", "conv_top_right", "conv_bottom_left", "conv_bottom_right", "conv_top", "conv_bottom",
         "conv_left", "conv_right")


def learned_regions(h, w, k, bc_x=1, bc_y=1):
    """Geometry of the nine banks on an h x w input: (fy, fx, ho, wo, {bank: (sy, sx, sh, sw, dy, dx)}) -- the frame widths,
    the output size and, per bank, the input rectangle it convolves (valid) and where its result lands in the output.  The
    strips are k + 1 (k = 5) or k wide, bc > 1 widens them by bc - 1.  The main bank comes first (the engine launches it on
    the conv kernels; the other eight are the frame of mc_learned_frame_*)."""
    pad_x = k + 1 + (bc_x - 1) if k == 5 else k + (bc_x - 1)
    pad_y = k + 1 + (bc_y - 1) if k == 5 else k + (bc_y - 1)
    fx, fy, mh, mw = pad_x - k + 1, pad_y - k + 1, h - k + 1, w - k + 1
    return fy, fx, mh + 2 * fy, mw + 2 * fx, {
        "conv": (0, 0, h, w, fy, fx),
        "conv_left": (0, 0, h, pad_x, fy, 0), "conv_right": (0, w - pad_x, h, pad_x, fy, fx + mw),
        "conv_bottom": (h - pad_y, 0, pad_y, w, 0, fx), "conv_top": (0, 0, pad_y, w, fy + mh, fx),
        "conv_bottom_left": (h - pad_y, 0, pad_y, pad_x, 0, 0),
        "conv_bottom_right": (h - pad_y, w - pad_x, pad_y, pad_x, 0, fx + mw),
        "conv_top_left": (0, 0, pad_y, pad_x, fy + mh, 0), "conv_top_right": (0, w - pad_x, pad_y, pad_x, fy + mh, fx + mw)}


@dataclass
class ConvShape:
    """Descriptors of one conv node at a given input size."""
    dgrad: bool                          # some source needs a gradient
    d: Optional[L.ConvDesc] = None       # forward
    dd: Optional[L.ConvDesc] = None      # input gradient (None when no source needs one)
    final_f32: bool = False              # the head writes its output in f32
    banks: Optional[dict] = None         # learned padding: bank -> (region, d, dd), the main bank first; d / dd stay None


def _conv_descs(N, h, w, cs, c_out, k, pad, mode, mc, mcg, sym=(0, 0, 0), out_f32=False, dgrad=True):
    """Forward descriptor of a conv over one or two concatenated sources of cs channels, and its input gradient: the same
    kernel on the padded domain (zero pad k - 1, rotated / transposed bank), its output split at cs[0] for two sources."""
    two = len(cs) > 1
    d = L.ConvDesc(N, h, w, cs[0], cs[1] if two else 0, c_out, k, pad, mode, mc, sym[0], 0, int(out_f32), sym[1], sym[2])
    if not dgrad:
        return d, None
    ho, wo = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    return d, L.ConvDesc(N, ho, wo, c_out, 0, sum(cs), k, k - 1, 0, mcg, 0, cs[0] if two else 0, 0)


def shape_walk(g: NetGraph, N: int, H: int, W: int, precision: str):
    """The graph's geometry at input size N x H x W, without touching a device: (size, grad, convs) = every tensor's (H, W),
    whether it needs a gradient, and a ConvShape per conv node (by index in g.nodes).  Engine.configure plans its buffers and
    launches on it."""
    mc, _ = DTYPES[precision]
    mcg = L.MC_BF16 if mc == L.MC_MIX16 else mc
    mode = L.PAD_MODES[g.pad_mode]
    size = {0: (H, W + 2 * g.in_pad_w)}
    grad = {0: g.input_grad}
    convs: Dict[int, ConvShape] = {}
    for i, node in enumerate(g.nodes):
        if node.kind == "up":
            size[node.out] = size[node.like] if node.like >= 0 else tuple(v * node.scale for v in size[node.src])
            grad[node.out] = True
            continue
        if node.kind == "pool":
            size[node.out] = tuple(v // node.f for v in size[node.src])
            grad[node.out] = grad[node.src]
            continue
        h, w = size[node.srcs[0]]
        if node.kind == "cat":
            if any(size[t] != (h, w) for t in node.srcs):
                raise ValueError("torch.cat operands must share H x W")
            size[node.out] = (h, w)
            grad[node.out] = True
            continue
        assert all(size[t] == (h, w) for t in node.srcs), "concat sources must agree in size"
        cs = [g.channels[t] for t in node.srcs]
        dgrad = any(grad[t] for t in node.srcs)
        k = node.k
        if node.spectral:
            assert len(cs) == 1, "a spectral layer takes one source tensor"
            if h < 8 or w < 8:
                raise ValueError(f"{node.name}: a spectral layer needs H >= 8 and W >= 8 (its two 4 x 4 mode blocks would overlap "
                                 f"or touch the Nyquist column), got {h}x{w}")
            ho, wo = h, w
            convs[i] = ConvShape(dgrad)
        elif node.learned:
            assert len(cs) == 1, "learned padding takes one source tensor"
            _, _, ho, wo, regs = learned_regions(h, w, k, node.bc_x, node.bc_y)
            if any(sy < 0 or sx < 0 or sh < k or sw < k for sy, sx, sh, sw, _, _ in regs.values()):
                raise ValueError(f"{node.name}: input {h}x{w} too small for learned padding")
            convs[i] = ConvShape(dgrad, banks={
                name: (r, *_conv_descs(N, r[2], r[3], cs, node.c_out, k, 0, L.PAD_MODES["zeros"], mc, mcg, (node.sym_h, 0, 0)))
                for name, r in regs.items()})
        else:
            ho, wo = h + 2 * node.pad - k + 1, w + 2 * node.pad - k + 1
            final_f32 = node.post == L.POST_NONE and node is g.nodes[-1] and mc != L.MC_F32 and node.c_out <= 16
            convs[i] = ConvShape(dgrad, *_conv_descs(N, h, w, cs, node.c_out, k, node.pad, mode, mc, mcg,
                                                     (node.sym_h, node.sym_v, node.sym_hv), final_f32, dgrad), final_f32)
        size[node.out] = (ho, wo)
        grad[node.out] = True
        if node.pool > 1:
            size[node.pooled] = (ho // node.pool, wo // node.pool)
            grad[node.pooled] = True
    return size, grad, convs


def iter_conv_descs(g: NetGraph, N: int, H: int, W: int, precision: str):
    """(name, forward descriptor, input-gradient descriptor or None) of every convolution launch of the graph at input size
    N x H x W, from the shape walk Engine.configure plans on (host-side checks: tests/test_abi_and_host.py compares every
    launch's bank reach with the bank's size)."""
    for i, c in shape_walk(g, N, H, W, precision)[2].items():
        if g.nodes[i].spectral:              # no convolution launch: a truncated DFT
            continue
        if c.banks is None:
            yield g.nodes[i].name, c.d, c.dd
        else:
            for name, (_, d, dd) in c.banks.items():
                yield g.nodes[i].name + name, d, dd


# ------------------------------------------------------------------------------------------------
# bicubic tap tables (nn.Upsample(mode='bicubic', align_corners=False), A = -0.75), built in f64
# ------------------------------------------------------------------------------------------------
def bicubic_tables(n_in: int, n_out: int):
    A = -0.75
    scale = n_in / n_out
    o = np.arange(n_out, dtype=np.float64)
    real = scale * (o + 0.5) - 0.5
    i0 = np.floor(real)
    t = real - i0

    def c1(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def c2(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    w = np.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], 1)
    idx = np.clip(i0[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1).astype(np.int32)
    # transposed (CSR over input index)
    lists = [dict() for _ in range(n_in)]
    for oo in range(n_out):
        for k in range(4):
            d = lists[idx[oo, k]]
            d[oo] = d.get(oo, 0.0) + w[oo, k]
    start = np.zeros(n_in + 1, np.int32)
    tj, tw = [], []
    for i in range(n_in):
        for oo in sorted(lists[i]):
            tj.append(oo)
            tw.append(lists[i][oo])
        start[i + 1] = len(tj)
    return (idx, w.astype(np.float32), start, np.asarray(tj, np.int32), np.asarray(tw, np.float32))


# ------------------------------------------------------------------------------------------------
# twiddle tables of the spectral layers, built in f64 from integer-reduced arguments
# ------------------------------------------------------------------------------------------------
def spectral_tables(H: int, W: int):
    """(rowtw [H][5][2], coltw [W][4][2]) f32: (cos, sin)(2 pi ((k h) mod H) / H) for |k1| = k = 0..4 and
    (cos, sin)(2 pi ((k2 w) mod W) / W) for k2 = 0..3."""
    def tab(n, ks):
        r = (np.arange(n, dtype=np.int64)[:, None] * np.arange(ks, dtype=np.int64)[None, :]) % n
        a = 2.0 * np.pi * r.astype(np.float64) / n
        return np.stack([np.cos(a), np.sin(a)], -1).astype(np.float32)
    return tab(H, 5), tab(W, 4)


# ------------------------------------------------------------------------------------------------
# engine
# ------------------------------------------------------------------------------------------------
@dataclass
class _T:            # runtime tensor
    C: int
    H: int = 0
    W: int = 0
    buf: Optional[torch.Tensor] = None
    requires_grad: bool = True
    # "normalise on load": the activated tensor is never materialised; consumers read the producer's raw conv output
    # `raw` and apply act(scale * y + shift) from `coef` ([N, CP, 4] table, None = activation only) while staging
    fused: bool = False
    raw: Optional[torch.Tensor] = None
    coef: Optional[torch.Tensor] = None
    act: int = 0


@dataclass(frozen=True)
class Switches:
    """The MANTLE_* environment switches, read once when an engine is built."""
    # bit 0: GroupNorm + activation applied by the consumers on load (conv, filter gradient, bicubic) instead of a
    # stand-alone pass that materialises the activated tensor; bit 1: the GroupNorm-backward reduction fused into the
    # epilogue of the input-gradient launch (single-consumer tensors).  0 = the round-1 unfused chain (A/B, tests).
    fuse: int
    # ... and only for tensors of at most this many pixels.  Measured on MI355X (CFG-3, B = 32): the MFMA kernels
    # of the two high-resolution levels are bound by vector-instruction issue, so GELU / GELU' evaluated inside them
    # costs more than the streaming pass it replaces (level-0 16->16 forward 117 -> 207 us against a 100 us pass);
    # at the deep levels the kernels are launch-latency bound and every fused pass is a launch saved.
    fuse_maxpix: int
    # "mixed" mode, round 3: the GroupNorm-backward reduction rides in the input-gradient launch of every eligible layer
    # whose launch is a row-reuse launch (the wide levels).  y is f16 there, so dz = dA * GELU'(z) and the two sums cost
    # 8.5 packed-f16 / mixed-precision instructions per element on the loader waves, beside the next stage's MFMAs,
    # instead of the ~25 f32 instructions that made the same fusion lose in round 2.
    fuse_dz_rr: bool
    # "mixed" mode: the filter-gradient launch of a layer whose dz comes from its consumer's input-gradient launch forms dY
    # from (dz, z) while it stages its tiles and stores it, instead of a stand-alone mc_gn_bwd_apply_dz pass
    # (single-chunk, single-group layers: 10->16 and 16->16).  0 selects the apply pass (A/B).
    wgrad_dz: bool
    # GroupNorm + activation of layers with at most this many pixels run as ONE launch per direction (statistics + apply
    # forward; reduce + finalize + apply backward).  MI355X, CFG-3: 64 x 64 and 32 x 32 layers 21 -> 11 us forward and
    # 38 -> 24 us backward; 128 x 128 layers break even (25 -> 24, 49 -> 53 us: 128 blocks do not fill the chip)
    gn_small_pix: int

    @classmethod
    def read(cls, precision):
        env, mixed = os.environ.get, precision == "mixed"
        return cls(int(env("MANTLE_FUSE", "0")), int(env("MANTLE_FUSE_MAXPIX", str(128 * 128))),
                   mixed and env("MANTLE_FUSE_DZ_RR", "1") != "0", mixed and env("MANTLE_WGRAD_DZ", "1") != "0",
                   int(env("MANTLE_GN_SMALL_PIX", str(64 * 64 + 4))))


# Routes: every choice between launches, made once by Engine._route before a buffer exists ("The engine's plan and routes")
class GnFwd(Enum):           # what follows a layer's conv launch
    NONE = "none"            # the final conv: nothing
    MEANS = "means"          # the final conv of a subtract_mean graph: its channel means (mc_gn_finalize)
    SMALL = "small"          # statistics + activation (+ pooling) in one launch (mc_gn_act_fwd_small)
    APPLY = "apply"          # mc_gn_finalize_coef (GroupNorm layers), then mc_gn_act_fwd
    FUSED = "fused"          # mc_gn_finalize_coef; consumers normalise on load, only a pooled tensor is materialised


class GnBwd(Enum):           # how a layer's dY is formed from the gradient of its activated output
    NONE = "none"            # the final conv: dY is the packed output gradient
    SMALL = "small"          # reduce + finalize + apply in one launch (mc_gn_act_bwd_small)
    APPLY = "apply"          # mc_gn_act_bwd_reduce + _finalize (GroupNorm layers), then mc_gn_act_bwd_apply
    DZ_APPLY = "dz_apply"    # dz and its sums came from the consumer's input-gradient launch: finalize + mc_gn_bwd_apply_dz
    DZ_WGRAD = "dz_wgrad"    # ... finalize_dz, and the filter-gradient launch forms dY (mc_conv2d_wgrad_dz)


class UpBwd(Enum):           # the bicubic adjoint
    WALK = "walk"
    TAPS = "taps"
    SEPARABLE = "separable"


DZ_ROUTES = (GnBwd.DZ_APPLY, GnBwd.DZ_WGRAD)


@dataclass(frozen=True)
class ConvRoute:
    need_part: bool          # the conv launch (or the pass after it) leaves per-tile sums of Y
    fused: bool              # the activated output is never materialised (_T.fused)
    gn_fwd: GnFwd
    gn_bwd: GnBwd
    epi: int = -1            # node index of the producer whose GroupNorm-backward reduction this layer's input-gradient launch carries
    dz_tiles: int = 0        # dz routes: partial-sum slots the consumer's conv tiles / conv tiles + fold blocks write
    dz_blocks: int = 0
    dz_n: bool = False       # dz routes: the finalize with one block per (group, sample) (_n), many slots per sample
    tiles: int = 0           # fixed-padding convs: tiles of the forward launch (<= 0: an unsupported configuration)


@dataclass(frozen=True)
class UpRoute:
    bwd: UpBwd
    maxtaps: Tuple[int, int]  # longest transposed tap list along y, x


@dataclass(slots=True, kw_only=True)
class LayerPlan:
    """What the three kinds of conv layer share: the raw output, its partial sums and the GroupNorm buffers of its route."""
    node: ConvNode
    route: ConvRoute
    tiles: int                               # partial-sum slots per sample
    coutp: int
    Y: torch.Tensor
    part: torch.Tensor
    need_dgrad: bool
    stats: Optional[torch.Tensor] = None     # GroupNorm layers: (mean, rstd) per (sample, group)
    m12: Optional[torch.Tensor] = None       # ... backward APPLY and the dz routes
    gpart: Optional[torch.Tensor] = None     # ... backward APPLY: per-block sums of the stand-alone reduction


@dataclass(slots=True, kw_only=True)
class ConvPlan(LayerPlan):
    op: ClassVar[str] = "conv"
    desc: L.ConvDesc
    ddesc: Optional[L.ConvDesc]
    bank: torch.Tensor
    wpart: torch.Tensor                      # filter-gradient partial slabs: ONE batched launch combines all layers'
    dbank: Optional[torch.Tensor] = None
    dxp: tuple = ()                          # input gradients on the padded domain, one per source
    coef: Optional[torch.Tensor] = None      # GroupNorm layers: (scale, shift, mean, rstd); padded channels stay 0
    pc: Optional[torch.Tensor] = None        # backward SMALL: per-channel sums for the batched dgamma / dbeta launch
    dz_part: Optional[torch.Tensor] = None   # dz routes: what the consumer's launch reduces into
    dz_pc: Optional[torch.Tensor] = None     # ... with the _n finalize
    dz_coef: Optional[torch.Tensor] = None   # DZ_WGRAD: (cA, cB, cC, mean) per (sample, channel); padded channels stay 0


@dataclass(slots=True, kw_only=True)
class LearnedPlan(LayerPlan):
    op: ClassVar[str] = "learned"
    ldesc: L.LearnedDesc
    desc: L.ConvDesc                         # the valid convolution on the whole input
    fdesc: L.ConvDesc                        # the main bank as launched forward (desc, or zero-padded straight into Y)
    ddesc: L.ConvDesc
    fy: int
    fx: int
    mh: int
    mw: int
    R: Optional[torch.Tensor]                # the valid result, where it has to be placed with mc_rect_copy
    dR: torch.Tensor
    dxl: Optional[torch.Tensor]
    bank: torch.Tensor
    dbank: Optional[torch.Tensor]
    wpart: torch.Tensor
    lbank: torch.Tensor
    ldbank: Optional[torch.Tensor]
    lws_bytes: int


@dataclass(slots=True, kw_only=True)
class SpectralPlan(LayerPlan):
    op: ClassVar[str] = "spectral"
    tabs: tuple
    apart: torch.Tensor                      # per-slot mode sums of the input / of dY
    xhat: torch.Tensor                       # modes of the input, kept for the backward pass
    mcoef: torch.Tensor                      # coefficients of the output / of the input gradient
    gbuf: torch.Tensor
    dxl: Optional[torch.Tensor]


@dataclass(slots=True, kw_only=True)
class UpPlan:
    op: ClassVar[str] = "up"
    node: UpNode
    route: UpRoute
    tabs: tuple
    dsrc: torch.Tensor
    bws: Optional[torch.Tensor] = None       # SEPARABLE: the f32 workspace between the two 1-D passes


@dataclass(slots=True, kw_only=True)
class PoolPlan:
    op: ClassVar[str] = "pool"
    node: PoolNode
    dsum: torch.Tensor


@dataclass(slots=True, kw_only=True)
class CatPlan:
    op: ClassVar[str] = "cat"
    node: CatNode
    gather: dict                             # tensor id -> (first channel, gradient buffer) of the operands gathered in backward


class _Backward:
    """The state of one backward call: what every tensor's gradient is read from, and the dz a consumer's input-gradient
    launch left for its producer.  Nothing of it outlives the call."""

    def __init__(self, params, grads, st):
        self.params, self.grads, self.st = params, grads, st
        self.srcs: Dict[int, list] = defaultdict(list)      # tensor id -> GradSrc list
        self.dz: Dict[int, L.GradSrc] = {}                   # output tensor id of the producer -> its dz
        self.gp_jobs = []                                    # GroupNorm parameter gradients of the one-launch layers

    def plain(self, tid, buf, t):
        self.srcs[tid].append(L.GradSrc(L.ptr(buf), L.GSRC_PLAIN, 0, 0, 1, t.H, t.W))


def _columns(rows, *types):
    """A list of job tuples as parallel ctypes arrays, one per column."""
    return [(t * len(rows))(*[r[k] for r in rows]) for k, t in enumerate(types)]


class Engine:
    """Executes a NetGraph.  `params` maps state-dict names to f32 device tensors;
    `grads` maps the same names to f32 device tensors that backward ACCUMULATES into."""

    def __init__(self, graph: NetGraph, precision: str = "fp32"):
        if precision not in DTYPES:
            raise ValueError(f"precision must be one of {list(DTYPES)}")
        L.load()
        self.g = graph
        self.precision = "fp32" if precision == "f32" else precision
        self.mc_dtype, self.t_dtype = DTYPES[precision]
        # gradient tensors: bf16 in the "mixed" mode (their range), the forward type otherwise
        self.mc_gdtype, self.g_dtype = (L.MC_BF16, torch.bfloat16) if self.mc_dtype == L.MC_MIX16 else (self.mc_dtype, self.t_dtype)
        self.shape = None
        self._frozen = False
        self._tables = {}
        self.sw = Switches.read(precision)
        self.plan, self.convs, self.learned, self.spectral = [], [], [], []
        self._probe, self._probe_pool = None, []
        # dropout (graphs with drop nodes only): the device state (seed_lo, seed_hi, step, 0) is allocated in configure();
        # the seed is kept here so that it survives a re-plan
        self.has_drop = any(n.kind == "conv" and n.drop > 0 for n in graph.nodes)
        self.drop_state = None
        self._drop_seed = 0
        self._drop_step = 0                  # a step set before configure() allocated drop_state: written there
        self._drop_on = False                # whether the last forward ran with dropout (its backward follows it)

    fuse = property(lambda self: self.sw.fuse)

    # -------------------------------------------------------------- dropout state
    def set_dropout_seed(self, seed: int):
        """64-bit seed of the dropout masks (low / high word = the Philox key); resets the step counter to 0."""
        self._drop_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._write_drop_state(0)

    def _write_drop_state(self, step: int):
        self._drop_step = 0 if self.drop_state is not None else int(step) & 0xFFFFFFFF
        if self.drop_state is not None:
            host = np.array([self._drop_seed & 0xFFFFFFFF, self._drop_seed >> 32, int(step) & 0xFFFFFFFF, 0], dtype=np.uint32)
            self.drop_state.copy_(torch.from_numpy(host.view(np.int32)))

    def dropout_step(self) -> int:
        """The device step counter: the number of training-mode forwards since the seed was set (host sync)."""
        if self.drop_state is None:
            return self._drop_step
        return int(self.drop_state[2].item()) & 0xFFFFFFFF

    def set_dropout_step(self, step: int):
        """Rewind / set the step counter (the trainer restores it after the warm-up pass of a graph capture).  Before the
        engine is planned the step is kept and written when configure() allocates the device state."""
        self._write_drop_state(step)

    def dropout_seed(self) -> int:
        """The 64-bit seed as set (the device state holds its two words)."""
        return self._drop_seed

    def _drop(self, node):
        """(entry-name suffix, trailing arguments) of a launch on this node's output: ("_drop", (mc_dropout,)) in a dropout
        pass of a dropout node -- backward regenerates the forward's mask from the same (seed, step, layer) -- else ("", ())."""
        if not (self._drop_on and node.drop > 0):
            return "", ()
        return "_drop", (C.byref(L.Dropout(L.ptr(self.drop_state), node.layer, L.dropout_keep16(node.drop))),)

    # -------------------------------------------------------------- planning
    def freeze(self):
        """Pin the configured shape: a captured HIP graph holds this engine's device pointers, so re-planning for another
        batch / grid size would leave the graph replaying freed memory.  Further calls with a different shape raise."""
        self._frozen = True

    def _cb8(self, c, h, w, grad=False):
        """An activation tensor (grad: a gradient tensor) in the CB8 layout."""
        return torch.empty((self.N, (c + 7) // 8, h, w, 8), dtype=self.g_dtype if grad else self.t_dtype, device=self.device)

    def _f32(self, *shape, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device=self.device)

    def _u8(self, nbytes):
        return torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def configure(self, N: int, H: int, W: int, device):
        if self.shape == (N, H, W, str(device)):
            return
        if self._frozen:
            raise RuntimeError(f"this engine is pinned to input shape {self.shape[:3]} by a captured HIP graph; got {(N, H, W)} "
                               "(use a separate module / engine instance, or an un-captured trainer, for another shape)")
        g = self.g
        if H % g.divisor or W % g.divisor:
            raise ValueError(f"input H, W must be divisible by {g.divisor}")
        self.device = device
        self.N = N
        size, grad, shapes = shape_walk(g, N, H, W, self.precision)
        self.T = T = {tid: _T(C=c, H=size[tid][0], W=size[tid][1], requires_grad=grad[tid]) for tid, c in g.channels.items()}
        self.mode = L.PAD_MODES[g.pad_mode]
        # consumers of every tensor (decides which activated tensors need not be materialised)
        self.cons = {tid: [] for tid in g.channels}
        for node in g.nodes:
            for i in (node.srcs if node.kind in ("conv", "cat") else [node.src]):
                self.cons[i].append(node)
        routes = self._route(size, shapes)   # every choice between launches, before the first buffer
        T[0].buf = self._cb8(T[0].C, T[0].H, T[0].W)
        self.plan = []
        self.prod = {}                       # tensor id -> plan record of the conv that produced it (full-resolution output)
        max_dy = 0
        for i, node in enumerate(g.nodes):
            if node.kind == "conv":
                o = T[node.out]
                plan = self._plan_spectral if node.spectral else self._plan_learned if node.learned else self._plan_conv
                e = plan(node, shapes[i], routes[i], [T[t] for t in node.srcs], o)
                if not o.fused:              # the activated output; a layer without activation: its raw output
                    o.buf = self._cb8(node.c_out, o.H, o.W) if node.post != L.POST_NONE else e.Y
                if node.pool > 1:
                    T[node.pooled].buf = self._cb8(node.c_out, T[node.pooled].H, T[node.pooled].W)
                max_dy = max(max_dy, N * e.coutp * o.H * o.W)
            else:
                T[node.out].buf = self._cb8(T[node.out].C, T[node.out].H, T[node.out].W)
                e = self._plan_up(node, routes[i]) if node.kind == "up" else getattr(self, "_plan_" + node.kind)(node)
            self.plan.append(e)
        # one output-gradient buffer for every layer: backward is one stream, so a layer's filter- and input-gradient
        # launches have read it before the next layer down writes its own
        self.dY = torch.empty(max_dy, dtype=self.g_dtype, device=device)
        self.convs = [e for e in self.plan if e.op == "conv"]
        self.learned = [e for e in self.plan if e.op == "learned"]
        self.spectral = [e for e in self.plan if e.op == "spectral"]
        # one filter-gradient workspace for the frames of every learned layer (backward is one stream)
        self.lws = self._u8(max([e.lws_bytes for e in self.learned] + [0]))
        last = self.plan[-1].node
        assert last.kind == "conv", "graph must end in a conv node"
        self.final_plain = last.post == L.POST_NONE
        assert self.final_plain or not g.subtract_mean
        fo = T[last.out]
        self.out_h, self.out_w = fo.H, fo.W - 2 * g.crop_w
        self.dOut = None if self.final_plain else self._cb8(fo.C, fo.H, fo.W, grad=True)
        self.chan_mean = self._f32(N, g.c_out) if g.subtract_mean else None
        self.gmean = self._f32(N, g.c_out) if g.subtract_mean else None
        if self.has_drop:
            self.drop_state = torch.zeros(4, dtype=torch.int32, device=device)
            self._write_drop_state(self._drop_step)      # (0 unless a restored step waited for this allocation)
        self.shape = (N, H, W, str(device))

    def _route(self, size, shapes):
        """The routing pass: node index -> ConvRoute / UpRoute for the whole graph, from the shapes, the switches and the
        library's host queries alone.  It runs before any buffer is allocated, so that "my consumer's input-gradient launch
        takes my reduction" is an input to a layer's own route; forward and backward switch on what it decides."""
        g, sw, ch = self.g, self.sw, self.g.channels
        routes, fused, prod, wdz_ok, epi, dz, tiles = {}, set(), {}, {}, {}, {}, {}
        for i, node in enumerate(g.nodes):
            if node.kind == "up":
                (h, w), (ho, wo) = size[node.src], size[node.out]
                maxtaps = tuple(int(np.diff(bicubic_tables(a, b)[2]).max()) for a, b in ((h, ho), (w, wo)))
                # scale factor > 3: the adjoint runs as two 1-D passes through an f32 workspace (tap lists too long
                # for the tiled kernel's window)
                sep = ho > 3 * h or wo > 3 * w
                routes[i] = UpRoute(UpBwd.SEPARABLE if sep else UpBwd.WALK if maxtaps[1] <= 12 else UpBwd.TAPS, maxtaps)
            if node.kind != "conv" or node.learned or node.spectral:
                continue
            tiles[i] = L.call("mc_conv_tiles", C.byref(shapes[i].d))
            if tiles[i] <= 0:                # _plan_conv raises when it comes to this node
                continue
            (h, w), (ho, wo), dd = size[node.srcs[0]], size[node.out], shapes[i].dd
            # this layer's filter-gradient launch may form dY from dz itself (mc_conv2d_wgrad_dz: "mixed", one input-channel
            # chunk, one output-channel group, sources read as they are), if its consumer leaves it a dz (below)
            wdz_ok[i] = (sw.wgrad_dz and self.mc_dtype == L.MC_MIX16 and node.post == L.POST_GN_ACT and node.c_out <= 16
                         and sum((ch[t] + 7) // 8 for t in node.srcs) <= 2 and not any(t in fused for t in node.srcs))
            cons = self.cons[node.out]
            fusable = all(c.kind == "up" or (c.kind == "conv" and not c.learned and not c.spectral) for c in cons)
            if ((sw.fuse & 1) and node.post != L.POST_NONE and fusable and (cons or node.pool > 1)
                    and ho * wo <= sw.fuse_maxpix and not node.drop):      # (a dropout layer's output is materialised)
                fused.add(node.out)
            prod[node.out] = i
            # GroupNorm-backward reduction fused into this layer's input-gradient epilogue: the source is the full-resolution
            # output of a conv + (GN) + act layer and this conv is its only consumer
            p = prod.get(node.srcs[0])
            if dd is None or p is None:
                continue
            dz_here = bool(sw.fuse & 2) and h * w <= sw.fuse_maxpix
            if (not dz_here and sw.fuse_dz_rr and g.act == "gelu"
                    and L.load().mc_conv_kernel_name(C.byref(dd)).decode().startswith("k_conv_rr")):
                dz_here = True
            pn = g.nodes[p]
            if (dz_here and len(node.srcs) == 1 and pn.post != L.POST_NONE and not pn.learned and not pn.spectral
                    and len(self.cons[node.srcs[0]]) == 1 and pn.pool == 1
                    and not pn.drop):               # (the epilogue's dz = dA act'(z) knows no mask)
                dtiles = L.call("mc_conv_tiles", C.byref(dd))
                epi[i], dz[p] = p, (dtiles, dtiles + L.call("mc_fold_blocks", h, w, node.pad, self.mode))
        for i, node in enumerate(g.nodes):
            if node.kind != "conv":
                continue
            (ho, wo), gn, final = size[node.out], node.post == L.POST_GN_ACT, node.post == L.POST_NONE
            pow2 = gn and (node.c_out // node.groups) in (1, 2, 4, 8)
            dz_tiles, dz_blocks = dz.get(i, (0, 0))
            # small layers: the GroupNorm backward (and, below, the forward) in one launch
            small = pow2 and ho * wo <= sw.gn_small_pix and not node.learned and not node.spectral
            if small and node.out not in fused and node.pool in (1, 2) and (sw.fuse == 0 or sw.fuse_dz_rr) and i not in dz:
                fwd = GnFwd.SMALL
            elif final:
                fwd = GnFwd.MEANS if g.subtract_mean else GnFwd.NONE
            else:
                fwd = GnFwd.FUSED if node.out in fused else GnFwd.APPLY
            if final:
                bwd = GnBwd.NONE
            elif i in dz:
                bwd = GnBwd.DZ_WGRAD if wdz_ok[i] else GnBwd.DZ_APPLY
            else:
                bwd = GnBwd.SMALL if small else GnBwd.APPLY
            routes[i] = ConvRoute(need_part=gn or (final and g.subtract_mean), fused=node.out in fused, gn_fwd=fwd, gn_bwd=bwd,
                                  epi=epi.get(i, -1), dz_tiles=dz_tiles, dz_blocks=dz_blocks,
                                  dz_n=pow2 and dz_blocks > 256,      # many slots per sample: one block per (group, sample)
                                  tiles=tiles.get(i, 0))
        return routes

    def _plan_gn(self, node, o, route, coutp):
        """GroupNorm statistics and the buffers of the backward form the route names, for any kind of conv layer."""
        if node.post != L.POST_GN_ACT:
            return {}
        N, bwd = self.N, route.gn_bwd
        return dict(stats=self._f32(N, node.groups, 2), m12=self._f32(N, node.groups, 2) if bwd is not GnBwd.SMALL else None,
                    gpart=self._f32(N, L.call("mc_gn_bwd_blocks", o.H, o.W), coutp, 2) if bwd is GnBwd.APPLY else None)

    def _plan_up(self, node, route):
        s, o = self.T[node.src], self.T[node.out]
        return UpPlan(node=node, route=route, tabs=(self._table(bicubic_tables, s.H, o.H), self._table(bicubic_tables, s.W, o.W)),
                      dsrc=self._cb8(s.C, s.H, s.W, grad=True),
                      bws=self._f32(self.N, (s.C + 7) // 8, s.H, o.W, 8) if route.bwd is UpBwd.SEPARABLE else None)

    def _plan_pool(self, node):
        o = self.T[node.out]
        return PoolPlan(node=node, dsum=self._cb8(o.C, o.H, o.W, grad=True))

    def _plan_cat(self, node):
        """backward: an operand that is exactly its own channel blocks of the concat (starts on a block boundary, and is the
        last operand or fills whole blocks) reads its slice of the concat's gradient in place; any other gets a buffer of
        its own, gathered by mc_cat_grad_gather (offset: the operand's first channel)."""
        T, o = self.T, self.T[node.out]
        gather, off = {}, 0
        for k, t in enumerate(node.srcs):
            c = T[t].C
            if T[t].requires_grad and (off % 8 or (k < len(node.srcs) - 1 and c % 8)):
                gather[t] = (off, self._cb8(c, o.H, o.W, grad=True))
            off += c
        return CatPlan(node=node, gather=gather)

    def _plan_conv(self, node, shape, route, srcs, o):
        """A convolution with fixed padding over one or two sources: the buffers of its route."""
        N, d, coutp, gn = self.N, shape.d, ((node.c_out + 7) // 8) * 8, node.post == L.POST_GN_ACT
        h, w, ho, wo = srcs[0].H, srcs[0].W, o.H, o.W
        tiles = route.tiles
        if tiles <= 0:
            raise L.MantleHipError(f"unsupported convolution configuration for {node.name} "
                                   f"({self.precision}, c_in={d.c_in0}+{d.c_in1}, c_out={node.c_out}, k={node.k})")
        dz = route.gn_bwd in DZ_ROUTES
        e = ConvPlan(node=node, route=route, desc=d, ddesc=shape.dd, tiles=tiles, coutp=coutp,
                     Y=self._f32(N, (node.c_out + 7) // 8, ho, wo, 8) if shape.final_f32 else self._cb8(node.c_out, ho, wo),
                     part=self._f32(N, tiles, coutp, 2), bank=self._u8(L.call("mc_packed_weight_bytes", C.byref(d), 0)),
                     need_dgrad=shape.dgrad, wpart=self._u8(L.call("mc_wgrad_partial_bytes", C.byref(d))),
                     coef=self._f32(N, coutp, 4, zero=True) if gn else None,
                     pc=self._f32(N, coutp, 2) if route.gn_bwd is GnBwd.SMALL else None,
                     dz_part=self._f32(N, route.dz_blocks, coutp, 2) if dz else None,
                     dz_pc=self._f32(N, coutp, 2) if route.dz_n else None,
                     dz_coef=self._f32(N, coutp, 4, zero=True) if route.gn_bwd is GnBwd.DZ_WGRAD else None,
                     **self._plan_gn(node, o, route, coutp))
        if shape.dgrad:
            hp, wp = h + 2 * node.pad, w + 2 * node.pad
            e.dbank = self._u8(L.call("mc_packed_weight_bytes", C.byref(d), 1))
            e.dxp = tuple(self._cb8(s.C, hp, wp, grad=True) for s in srcs)
        o.fused = route.fused
        if o.fused:
            o.raw, o.coef, o.act = e.Y, e.coef, L.ACTS[self.g.act]
        self.prod[node.out] = e
        return e

    # -------------------------------------------------------------- learned padding (BoundaryLearnedConvolution2D)
    def _plan_learned(self, node, shape, route, srcs, o):
        """The main bank on the library's conv kernels, the frame of the eight border banks on the mc_learned_frame_* kernels,
        which read the input / the output gradient in place (reference pytorch_networks_convae.py:1022-1065).  The gradient
        w.r.t. the input needs no padded domain: the adjoint of a valid convolution is exactly input-sized."""
        (s,), N = srcs, self.N
        reg, d, dd = shape.banks["conv"]                          # the valid convolution on the whole input
        ld = L.LearnedDesc(N, s.H, s.W, s.C, node.c_out, node.k, node.bc_x, node.bc_y, self.mc_dtype, node.sym_h)
        if L.call("mc_learned_validate", C.byref(ld)) != 0 or L.call("mc_conv_tiles", C.byref(d)) <= 0:
            raise L.MantleHipError(f"unsupported learned-padding configuration for {node.name} ({self.precision}, "
                                   f"c_in={s.C}, c_out={node.c_out}, k={node.k}, input {s.H}x{s.W})")
        fy, fx, mh, mw = reg[4], reg[5], dd.h, dd.w
        # square frame: the main bank as a zero-padded convolution straight into Y -- its interior is the valid result, its
        # frame is overwritten by the frame launch; otherwise the valid result is placed with one mc_rect_copy
        fd = d
        if fx == fy and fx <= node.k - 1:
            fd = L.ConvDesc(N, s.H, s.W, s.C, 0, node.c_out, node.k, fx, L.PAD_MODES["zeros"], self.mc_dtype, node.sym_h, 0, 0)
            if L.call("mc_conv_tiles", C.byref(fd)) <= 0:
                fd = d
        coutp = ((node.c_out + 7) // 8) * 8
        tiles = min(64, o.H)
        dg = s.requires_grad
        e = LearnedPlan(node=node, route=route, ldesc=ld, desc=d, fdesc=fd, ddesc=dd, fy=fy, fx=fx, mh=mh, mw=mw, tiles=tiles,
                        coutp=coutp, Y=self._cb8(node.c_out, o.H, o.W), R=None if fd is not d else self._cb8(node.c_out, mh, mw),
                        dR=self._cb8(node.c_out, mh, mw, grad=True), part=self._f32(N, tiles, coutp, 2), need_dgrad=dg,
                        dxl=self._cb8(s.C, s.H, s.W, grad=True) if dg else None,
                        bank=self._u8(L.call("mc_packed_weight_bytes", C.byref(fd), 0)),
                        dbank=self._u8(L.call("mc_packed_weight_bytes", C.byref(d), 1)) if dg else None,
                        wpart=self._u8(L.call("mc_wgrad_partial_bytes", C.byref(d))),
                        lbank=self._u8(L.call("mc_learned_bank_bytes", C.byref(ld), 0)),
                        ldbank=self._u8(L.call("mc_learned_bank_bytes", C.byref(ld), 1)) if dg else None,
                        lws_bytes=L.call("mc_learned_wgrad_workspace_bytes", C.byref(ld)), **self._plan_gn(node, o, route, coutp))
        return e

    def _fwd_learned(self, e, params, st):
        node, N, src = e.node, self.N, self.T[e.node.srcs[0]]
        bias = self._param(params, node.name + "learnable_bias")
        o_h, o_w = e.Y.shape[2], e.Y.shape[3]
        main = e.Y if e.R is None else e.R
        L.call("mc_conv2d", C.byref(e.fdesc), L.ptr(src.buf), None, L.ptr(e.bank), L.ptr(bias), L.ptr(main), None, None, st)
        if e.R is not None:
            L.call("mc_rect_copy", L.ptr(e.R), e.mh, e.mw, 0, 0, L.ptr(e.Y), o_h, o_w, e.fy, e.fx, e.mh, e.mw,
                   N, node.c_out, 0, self.mc_dtype, st)
        L.call("mc_learned_frame_fwd", C.byref(e.ldesc), L.ptr(src.buf), L.ptr(e.lbank), L.ptr(bias), L.ptr(e.Y), st)
        if e.route.need_part:
            L.call("mc_gn_partials", L.ptr(e.Y), N, node.c_out, o_h, o_w, self.mc_dtype, e.tiles, L.ptr(e.part), st)
        self._fwd_gn(e, params, st)

    def _bwd_learned(self, e, bk):
        """The main bank's filter gradient joins the batched combine at the end of backward (e.wpart); its input gradient
        initialises dxl, the frame launch adds the eight border banks' to the border bands of dxl."""
        self._bwd_gn(e, bk)
        node, N, src, dY, grads, st = e.node, self.N, self.T[e.node.srcs[0]], self.dY, bk.grads, bk.st
        o_h, o_w = e.Y.shape[2], e.Y.shape[3]
        L.call("mc_rect_copy", L.ptr(dY), o_h, o_w, e.fy, e.fx, L.ptr(e.dR), e.mh, e.mw, 0, 0, e.mh, e.mw, N,
               node.c_out, 0, self.mc_gdtype, st)
        L.call("mc_conv2d_wgrad", C.byref(e.desc), L.ptr(src.buf), None, L.ptr(e.dR), L.ptr(e.wpart), st)
        dws = (C.c_void_p * 8)(*[L.ptr(grads[node.name + b + ".weight"]) for b in L.LEARNED_FRAME_BANKS])
        L.call("mc_learned_frame_wgrad", C.byref(e.ldesc), L.ptr(src.buf), L.ptr(dY), L.ptr(self.lws), dws,
               L.ptr(grads[node.name + "learnable_bias"]), st)
        if e.need_dgrad:
            L.call("mc_conv2d", C.byref(e.ddesc), L.ptr(e.dR), None, L.ptr(e.dbank), None, L.ptr(e.dxl), None, None, st)
            L.call("mc_learned_frame_dgrad", C.byref(e.ldesc), L.ptr(dY), L.ptr(e.ldbank), L.ptr(e.dxl), st)
            bk.plain(node.srcs[0], e.dxl, src)

    # -------------------------------------------------------------- spectral layers (SpectralConv2d)
    def _plan_spectral(self, node, shape, route, srcs, o):
        """A truncated DFT (csrc/spectral.hip): analysis of the materialised input, channel mixing in mode space, synthesis into
        the raw output Y with the GroupNorm partials.  The GroupNorm / activation / pooling launches after it are the generic
        ones; its input gradient is the input-sized buffer dxl, as for a learned-padding layer."""
        (s,), N = srcs, self.N
        slots = L.call("mc_spectral_slots", s.H, s.W)
        if slots <= 0:
            raise L.MantleHipError(f"unsupported spectral layer {node.name}: input {s.H}x{s.W}")
        cinp, coutp = ((s.C + 7) // 8) * 8, ((node.c_out + 7) // 8) * 8
        cmax = max(cinp, coutp)
        e = SpectralPlan(node=node, route=route, tiles=slots, coutp=coutp, Y=self._cb8(node.c_out, o.H, o.W),
                         part=self._f32(N, slots, coutp, 2), tabs=self._table(spectral_tables, s.H, s.W), need_dgrad=s.requires_grad,
                         apart=self._f32(N, slots, cmax, 32, 2), xhat=self._f32(N, cinp, 32, 2), mcoef=self._f32(N, cmax, 32, 2),
                         gbuf=self._f32(N, coutp, 32, 2), dxl=self._cb8(s.C, s.H, s.W, grad=True) if s.requires_grad else None,
                         **self._plan_gn(node, o, route, coutp))
        return e

    def _fwd_spectral(self, e, params, st):
        node, N, src = e.node, self.N, self.T[e.node.srcs[0]]
        w1, w2 = self._param(params, node.name + "weights1"), self._param(params, node.name + "weights2")
        rowtw, coltw = e.tabs
        L.call("mc_spectral_analyze", L.ptr(src.buf), N, src.C, src.H, src.W, self.mc_dtype, L.ptr(rowtw), L.ptr(coltw),
               L.ptr(e.apart), st)
        L.call("mc_spectral_mix_fwd", L.ptr(e.apart), N, e.tiles, src.C, node.c_out, src.H * src.W, L.ptr(w1), L.ptr(w2),
               L.ptr(e.xhat), L.ptr(e.mcoef), st)
        L.call("mc_spectral_synthesize", L.ptr(e.mcoef), N, node.c_out, src.H, src.W, self.mc_dtype, L.ptr(rowtw), L.ptr(coltw),
               L.ptr(e.Y), L.ptr(e.part) if e.route.need_part else None, st)
        self._fwd_gn(e, params, st)

    def _bwd_spectral(self, e, bk):
        """dY -> its modes -> the two weight gradients (accumulated, samples in order) and the coefficients of the input
        gradient -> dxl."""
        self._bwd_gn(e, bk)
        node, N, src, dY, grads, st = e.node, self.N, self.T[e.node.srcs[0]], self.dY, bk.grads, bk.st
        w1, w2 = self._param(bk.params, node.name + "weights1"), self._param(bk.params, node.name + "weights2")
        rowtw, coltw = e.tabs
        L.call("mc_spectral_analyze", L.ptr(dY), N, node.c_out, src.H, src.W, self.mc_gdtype, L.ptr(rowtw), L.ptr(coltw),
               L.ptr(e.apart), st)
        L.call("mc_spectral_mix_bwd", L.ptr(e.apart), N, e.tiles, src.C, node.c_out, src.H * src.W, L.ptr(w1), L.ptr(w2),
               L.ptr(e.xhat), L.ptr(e.gbuf), L.ptr(grads[node.name + "weights1"]), L.ptr(grads[node.name + "weights2"]),
               L.ptr(e.mcoef) if e.need_dgrad else None, st)
        if e.need_dgrad:
            L.call("mc_spectral_synthesize", L.ptr(e.mcoef), N, src.C, src.H, src.W, self.mc_gdtype, L.ptr(rowtw), L.ptr(coltw),
                   L.ptr(e.dxl), None, st)
            bk.plain(node.srcs[0], e.dxl, src)

    def input_grad(self):
        """input_grad_cb8() as an NCHW f32 tensor (what the autograd bridge returns for the input)."""
        dxl, s = self.input_grad_cb8(), self.T[0]
        dx = torch.empty((self.N, s.C, s.H, s.W), dtype=torch.float32, device=dxl.device)
        L.call("mc_unpack_nchw", L.ptr(dxl), self.N, s.C, s.H, s.W, 0, None, self.mc_gdtype, L.ptr(dx), L.stream())
        return dx

    def input_grad_cb8(self):
        """d(loss)/d(input) of a graph built with input_grad=True, as backward left it: CB8 [N][C8][H][W][8] in the gradient
        type (the first node must be a learned-padding or spectral layer reading the input)."""
        if not self.g.input_grad or getattr(self.plan[0], "dxl", None) is None:
            raise RuntimeError("this graph produces no input gradient")
        return self.plan[0].dxl

    def _table(self, build, *size):
        """The host tables build(*size) (bicubic_tables, spectral_tables) as device tensors, built once per size."""
        key = (build, *size)
        if key not in self._tables:
            self._tables[key] = tuple(torch.from_numpy(a).to(self.device) for a in build(*size))
        return self._tables[key]

    # -------------------------------------------------------------- forward
    def output_cb8(self):
        """The last convolution's output as the forward pass left it, for consumers that read the CB8 layout themselves
        (StokesLoss.evaluate(cb8=...)): (buffer [N][C8][H][W + 2 crop][8] f32, per-(sample, channel) spatial means or None,
        crop, (N, C, H, W)); None when the head does not end in an f32 tensor."""
        fo = self.T[self.plan[-1].node.out]
        if fo.buf is None or fo.buf.dtype != torch.float32 or fo.C != self.g.c_out:
            return None
        return fo.buf, (self.chan_mean if self.g.subtract_mean else None), self.g.crop_w, (self.N, self.g.c_out, self.out_h, self.out_w)

    def forward(self, x: torch.Tensor, params: Dict[str, torch.Tensor], chan_scale=None, out=None, unpack=True,
                drop=False) -> torch.Tensor:
        """x: [N, >= c_in, H, W] f32 device tensor (extra trailing channels are ignored)
        -> [N, c_out, H', W'] f32.  chan_scale: optional [c_in] f32 per-channel input scale.  out: optional preallocated
        result (the fused trainer passes one so that a captured step allocates nothing).  drop: training mode -- the
        graph's dropout layers are active, and the device step counter advances first (a one-thread kernel on the stream,
        so every replay of a captured step draws a new mask); graphs without dropout layers ignore it."""
        L.require_cuda(x, "network input")
        if x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        N, Ci, H, W = x.shape
        if Ci < self.g.c_in:
            raise ValueError(f"expected at least {self.g.c_in} input channels, got {Ci}")
        self.configure(N, H, W, x.device)
        st = L.stream()
        g, T = self.g, self.T
        self._drop_on = bool(drop) and self.has_drop
        if self._drop_on:
            L.call("mc_dropout_advance", L.ptr(self.drop_state), st)
        L.call("mc_pack_nchw", L.ptr(x), N, g.c_in, Ci, H, W, g.in_pad_w, self.mode, L.ptr(chan_scale), self.mc_dtype,
               L.ptr(T[0].buf), st)
        self._pack_all_banks(params, st)
        for e in self.plan:
            getattr(self, "_fwd_" + e.op)(e, params, st)
        fo = T[self.plan[-1].node.out]
        if not unpack and self.output_cb8() is not None:      # the caller reads output_cb8() (no NCHW copy of the output)
            return None
        if out is None:
            out = torch.empty((N, g.c_out, self.out_h, self.out_w), dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != (N, g.c_out, self.out_h, self.out_w) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous f32 tensor of the network's output shape")
        out_dt = L.MC_F32 if fo.buf.dtype == torch.float32 else self.mc_dtype
        L.call("mc_unpack_nchw", L.ptr(fo.buf), N, fo.C, fo.H, fo.W, g.crop_w, L.ptr(self.chan_mean), out_dt,
               L.ptr(out), st)
        return out

    def _fwd_pool(self, e, params, st):
        s, o = self.T[e.node.src], self.T[e.node.out]
        L.call("mc_avgpool_fwd", L.ptr(s.buf), self.N, s.C, s.H, s.W, e.node.f, self.mc_dtype, L.ptr(o.buf), st)

    def _fwd_cat(self, e, params, st):
        srcs, o = [self.T[i] for i in e.node.srcs], self.T[e.node.out]
        ptrs, cs = _columns([(L.ptr(t.buf), t.C) for t in srcs], C.c_void_p, C.c_int32)
        L.call("mc_concat_cb8", ptrs, cs, len(srcs), self.N, o.H, o.W, self.mc_dtype, L.ptr(o.buf), st)

    def _fwd_up(self, e, params, st):
        s, o, N = self.T[e.node.src], self.T[e.node.out], self.N
        (iy, wy, *_), (ix, wx, *_) = e.tabs
        # a fused source: the producer's GroupNorm + activation are applied while the input window is staged
        sfx, src = ("_act", (L.ptr(s.raw), L.ptr(s.coef), s.act)) if s.fused else ("", (L.ptr(s.buf),))
        L.call("mc_bicubic_fwd" + sfx, *src, N, s.C, s.H, s.W, o.H, o.W, L.ptr(iy), L.ptr(wy), L.ptr(ix), L.ptr(wx),
               self.mc_dtype, L.ptr(o.buf), st)

    def _fwd_conv(self, e, params, st):
        node, d = e.node, e.desc
        b = self._param(params, node.name + "bias")
        self._probe_begin()
        x0, x1, pro = self._sources([self.T[i] for i in node.srcs])
        L.call("mc_conv2d_fused", C.byref(d), x0, x1, pro, L.ptr(e.bank), L.ptr(b), L.ptr(e.Y), None,
               L.ptr(e.part) if e.route.need_part else None, None, st)
        self._probe_end(d, "fwd " + node.name)
        self._fwd_gn(e, params, st)

    def _fwd_gn(self, e, params, st):
        """What follows the conv launch of any kind of conv layer: the route's GroupNorm / activation / pooling form."""
        node, N, o, form = e.node, self.N, self.T[e.node.out], e.route.gn_fwd
        if form is GnFwd.NONE:
            return
        if form is GnFwd.MEANS:
            L.call("mc_gn_finalize", L.ptr(e.part), N, e.tiles, node.c_out, 1, o.H * o.W, 1e-5, None, L.ptr(self.chan_mean), st)
            return
        gamma, beta = self._gn_params(node, params)
        act, pooled = L.ACTS[self.g.act], (self.T[node.pooled].buf if node.pool > 1 else None)
        sfx, dra = self._drop(node)
        if form is GnFwd.SMALL:
            L.call("mc_gn_act_fwd_small" + sfx, L.ptr(e.Y), L.ptr(e.part), e.tiles, N, node.c_out, o.H, o.W, node.groups, 1e-5,
                   L.ptr(gamma), L.ptr(beta), act, node.pool, self.mc_dtype, L.ptr(e.stats), L.ptr(o.buf), L.ptr(pooled), *dra, st)
            return
        if node.post == L.POST_GN_ACT:
            # (mean, rstd) per (sample, group) + the (scale, shift, mean, rstd) table consumers normalise on load with
            L.call("mc_gn_finalize_coef", L.ptr(e.part), N, e.tiles, node.c_out, node.groups, o.H * o.W, 1e-5,
                   L.ptr(gamma), L.ptr(beta), L.ptr(e.stats), L.ptr(getattr(e, "coef", None)), st)
        if form is GnFwd.APPLY or node.pool > 1:      # FUSED: only the pooled tensor is materialised (o.buf is None)
            L.call("mc_gn_act_fwd" + sfx, L.ptr(e.Y), N, node.c_out, o.H, o.W, node.groups, L.ptr(e.stats), L.ptr(gamma),
                   L.ptr(beta), node.post, act, node.pool, self.mc_dtype, L.ptr(o.buf), L.ptr(pooled), *dra, st)

    def _gn_params(self, node, params):
        """(gamma, beta) of the node's GroupNorm, (None, None) without one."""
        if not node.gn_name:
            return None, None
        return self._param(params, node.gn_name + "weight"), self._param(params, node.gn_name + "bias")

    @staticmethod
    def _sources(srcs):
        """(x0, x1, prologue) of a conv's one or two sources: a fused tensor is read as the producer's raw conv output with
        its (scale, shift) table and activation; anything else as it is."""
        ptrs = [L.ptr(t.raw if t.fused else t.buf) for t in srcs] + [None]
        if not any(t.fused for t in srcs):
            return ptrs[0], ptrs[1], None
        t1 = srcs[1] if len(srcs) > 1 else None
        pro = L.ConvPrologue(L.ptr(srcs[0].coef) if srcs[0].fused else None,
                             L.ptr(t1.coef) if (t1 is not None and t1.fused) else None,
                             srcs[0].act if srcs[0].fused else 0, t1.act if (t1 is not None and t1.fused) else 0)
        return ptrs[0], ptrs[1], C.byref(pro)

    @staticmethod
    def _param(params, name):
        p = params[name]
        if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
            raise RuntimeError(f"parameter {name} must be a contiguous f32 device tensor")
        return p

    # -------------------------------------------------------------- backward
    def backward(self, gout: torch.Tensor, params: Dict[str, torch.Tensor], grads: Dict[str, torch.Tensor], gsum=None):
        """gout: d(loss)/d(output) [N, c_out, H', W'] f32.  Accumulates parameter gradients into `grads`.
        gsum: (per-block sums [N, blocks, 4] of gout's channel planes, blocks) from the producer of gout
        (StokesLoss.gradient_sums()): the spatial means of gout are then taken from them instead of a pass over gout."""
        L.require_cuda(gout, "output gradient")
        gout = gout.contiguous().float()
        g, N = self.g, self.N
        st = L.stream()
        bk = _Backward(params, grads, st)
        last = self.plan[-1].node
        fo = self.T[last.out]
        mean = None
        if g.subtract_mean:
            if gsum is not None and g.c_out <= 4 and tuple(gsum[0].shape) == (N, gsum[1], 4):
                L.call("mc_partial_sums_finalize", L.ptr(gsum[0]), N, gsum[1], g.c_out, 1.0 / (fo.H * fo.W), L.ptr(self.gmean), st)
            else:
                L.call("mc_sum_hw", L.ptr(gout), N * g.c_out, self.out_h * self.out_w, 1.0 / (fo.H * fo.W),
                       L.ptr(self.gmean), st)
            mean = self.gmean
        gdst = self.dY if self.final_plain else self.dOut        # self.dY: every layer's output gradient (see configure)
        L.call("mc_pack_grad_nchw", L.ptr(gout), N, g.c_out, fo.H, fo.W, g.crop_w, L.ptr(mean), self.mc_gdtype,
               L.ptr(gdst), st)
        if not self.final_plain:
            bk.plain(last.out, self.dOut, fo)
        for e in reversed(self.plan):
            getattr(self, "_bwd_" + e.op)(e, bk)
        if bk.gp_jobs:
            L.call("mc_gn_param_grads_batched", *_columns(bk.gp_jobs, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p),
                   len(bk.gp_jobs), st)
        # one launch combines every layer's partial slabs, folds mirrored filters and accumulates into the gradients
        # (a learned layer's main bank: its valid convolution; the shared bias takes its interior share here)
        jobs = [(e.desc, L.ptr(e.wpart), L.ptr(grads[e.node.name + w]), L.ptr(grads[e.node.name + b]))
                for es, w, b in ((self.convs, "weight", "bias"), (self.learned, "conv.weight", "learnable_bias")) for e in es]
        if jobs:
            L.call("mc_conv2d_wgrad_finalize_batched", *_columns(jobs, L.ConvDesc, C.c_void_p, C.c_void_p, C.c_void_p), len(jobs), st)

    def _bwd_cat(self, e, bk):
        """The gradient of the concatenated tensor is one buffer; an aligned operand reads its channel-block slice, an
        unaligned one its own buffer gathered from it (see _plan_cat)."""
        node, T, N, o = e.node, self.T, self.N, self.T[e.node.out]
        assert len(bk.srcs[node.out]) == 1, "a concatenated tensor feeds exactly one conv"
        q = bk.srcs[node.out][0]
        off = 0
        for i in node.srcs:
            t = T[i]
            if i in e.gather:
                c_off, buf = e.gather[i]
                L.call("mc_cat_grad_gather", C.byref(q), o.C, c_off, t.C, N, t.H, t.W, self.mc_gdtype, L.ptr(buf), bk.st)
                bk.plain(i, buf, t)
            elif t.requires_grad:
                bk.srcs[i].append(L.GradSrc(q.ptr, q.kind, q.pad, q.pad_mode, q.pool, q.hs, q.ws, (o.C + 7) // 8, off // 8))
            off += t.C

    def _bwd_pool(self, e, bk):
        """d(src) += AvgPool adjoint of d(out); d(out) has one source (the conv it feeds) or two (+ the next pooling level)."""
        node, s, o = e.node, self.T[e.node.src], self.T[e.node.out]
        gs = bk.srcs[node.out]
        assert 1 <= len(gs) <= 2
        if not s.requires_grad:
            return
        q = gs[0]
        if len(gs) == 1 and q.kind == L.GSRC_PADFOLD and q.c8_total == 0:
            bk.srcs[node.src].append(L.GradSrc(q.ptr, L.GSRC_PADFOLD_POOL, q.pad, q.pad_mode, node.f, o.H, o.W))
        else:
            g1 = C.byref(gs[1]) if len(gs) > 1 else None
            L.call("mc_gsrc_sum", C.byref(q), g1, self.N, o.C, o.H, o.W, self.mc_gdtype, L.ptr(e.dsum), bk.st)
            bk.srcs[node.src].append(L.GradSrc(L.ptr(e.dsum), L.GSRC_PLAIN_POOL, 0, 0, node.f, o.H, o.W))

    def _bwd_up(self, e, bk):
        node, s, o, N, st = e.node, self.T[e.node.src], self.T[e.node.out], self.N, bk.st
        assert len(bk.srcs[node.out]) == 1, "an upsampled tensor feeds exactly one conv"
        (iy, wy, tys, tyj, tyw), (_, _, txs, txj, txw) = e.tabs
        head, (my, mx) = (C.byref(bk.srcs[node.out][0]), N, s.C, s.H, s.W, o.H, o.W), e.route.maxtaps
        taps = (L.ptr(tys), L.ptr(tyj), L.ptr(tyw), L.ptr(txs), L.ptr(txj), L.ptr(txw))
        if e.route.bwd is UpBwd.WALK:
            L.call("mc_bicubic_bwd_walk", *head, L.ptr(iy), L.ptr(wy), L.ptr(tys), L.ptr(tyj), L.ptr(txs), L.ptr(txj), L.ptr(txw),
                   mx, self.mc_gdtype, L.ptr(e.dsrc), st)
        elif e.route.bwd is UpBwd.SEPARABLE:
            L.call("mc_bicubic_bwd_separable", *head, *taps, self.mc_gdtype, L.ptr(e.bws), L.ptr(e.dsrc), st)
        else:
            L.call("mc_bicubic_bwd_taps", *head, *taps, my, mx, self.mc_gdtype, L.ptr(e.dsrc), st)
        bk.plain(node.src, e.dsrc, s)

    def _bwd_gn(self, e, bk):
        """dY of any kind of conv layer from the gradient of its activated output, in the route's form."""
        node, N, o, form, dY, st = e.node, self.N, self.T[e.node.out], e.route.gn_bwd, self.dY, bk.st
        if form is GnBwd.NONE:
            return
        gn, act = node.post == L.POST_GN_ACT, L.ACTS[self.g.act]
        gamma, beta = self._gn_params(node, bk.params)
        dgamma, dbeta = (L.ptr(bk.grads[node.gn_name + "weight"]), L.ptr(bk.grads[node.gn_name + "bias"])) if gn else (None, None)
        if form in DZ_ROUTES:
            # dz = dA * act'(z) and its partial sums were produced by the consumer's input-gradient launch
            assert not bk.srcs[node.out], f"{node.name}: fused dz and separate gradient sources"
            wdz, dz = form is GnBwd.DZ_WGRAD, bk.dz[node.out]
            if gn:
                # _n: per-channel sums, whose dgamma / dbeta join the batched launch at the end of backward
                n, dst = ("_n", (L.ptr(e.dz_pc),)) if e.route.dz_n else ("", (dgamma, dbeta))
                dzs, tab = ("_dz", (L.ptr(e.coef), L.ptr(e.dz_coef))) if wdz else ("", ())
                L.call("mc_gn_act_bwd_finalize" + n + dzs, L.ptr(e.dz_part), N, e.route.dz_blocks, node.c_out, node.groups,
                       o.H * o.W, L.ptr(gamma), L.ptr(e.m12), *dst, *tab, st)
                if e.route.dz_n:
                    bk.gp_jobs.append((L.ptr(e.dz_pc), N, node.c_out, dgamma, dbeta))
            if wdz:              # dY is formed by the filter-gradient launch
                x0, x1, _ = self._sources([self.T[i] for i in node.srcs])
                L.call("mc_conv2d_wgrad_dz", C.byref(e.desc), x0, x1, C.byref(dz), L.ptr(e.Y), L.ptr(e.dz_coef),
                       L.ptr(dY), L.ptr(e.wpart), st)
            else:
                L.call("mc_gn_bwd_apply_dz", C.byref(dz), L.ptr(e.Y), N, node.c_out, o.H, o.W, max(node.groups, 1),
                       L.ptr(e.coef) if gn else None, L.ptr(e.m12), self.mc_dtype, L.ptr(dY), st)
            return
        gs = list(bk.srcs[node.out])
        if node.pool > 1:
            p = self.T[node.pooled]
            for q in bk.srcs[node.pooled]:
                assert q.kind in (L.GSRC_PADFOLD, L.GSRC_PLAIN) and q.c8_total == 0, "a pooled tensor feeds exactly one conv"
                kind = L.GSRC_PADFOLD_POOL if q.kind == L.GSRC_PADFOLD else L.GSRC_PLAIN_POOL   # (PLAIN: learned-padding conv)
                gs.append(L.GradSrc(q.ptr, kind, q.pad, q.pad_mode, node.pool, p.H, p.W))
        assert 1 <= len(gs) <= 2, f"{node.name}: {len(gs)} gradient sources"
        g0, g1 = C.byref(gs[0]), (C.byref(gs[1]) if len(gs) > 1 else None)
        sfx, dra = self._drop(node)
        if form is GnBwd.SMALL:
            L.call("mc_gn_act_bwd_small" + sfx, L.ptr(e.Y), N, node.c_out, o.H, o.W, node.groups, L.ptr(e.stats),
                   L.ptr(gamma), L.ptr(beta), act, self.mc_dtype, g0, g1, L.ptr(dY), L.ptr(e.pc), *dra, st)
            bk.gp_jobs.append((L.ptr(e.pc), N, node.c_out, dgamma, dbeta))
            return
        if gn:
            L.call("mc_gn_act_bwd_reduce" + sfx, L.ptr(e.Y), N, node.c_out, o.H, o.W, node.groups, L.ptr(e.stats), L.ptr(gamma),
                   L.ptr(beta), node.post, act, self.mc_dtype, g0, g1, L.ptr(e.gpart), *dra, st)
            L.call("mc_gn_act_bwd_finalize", L.ptr(e.gpart), N, e.gpart.shape[1], node.c_out, node.groups, o.H * o.W, L.ptr(gamma),
                   L.ptr(e.m12), dgamma, dbeta, st)
        L.call("mc_gn_act_bwd_apply" + sfx, L.ptr(e.Y), N, node.c_out, o.H, o.W, node.groups, L.ptr(e.stats), L.ptr(e.m12),
               L.ptr(gamma), L.ptr(beta), node.post, act, self.mc_dtype, g0, g1, L.ptr(dY), *dra, st)

    def _bwd_conv(self, e, bk):
        """dY, the filter-gradient partials (combined at the end of backward) and the input gradients on the padded domain."""
        self._bwd_gn(e, bk)
        node, N, dY, dxp, st = e.node, self.N, self.dY, e.dxp, bk.st
        srcs = [self.T[i] for i in node.srcs]
        if e.route.gn_bwd is not GnBwd.DZ_WGRAD:
            x0, x1, pro = self._sources(srcs)
            L.call("mc_conv2d_wgrad_fused", C.byref(e.desc), x0, x1, pro, L.ptr(dY), L.ptr(e.wpart), st)
        if not e.need_dgrad:
            return
        if e.route.epi >= 0:
            # the source's GroupNorm-backward reduction rides in this launch: dz and its partial sums instead of dA
            pe, s0, act = self.plan[e.route.epi], srcs[0], L.ACTS[self.g.act]
            coef, blocks = (L.ptr(pe.coef) if pe.node.post == L.POST_GN_ACT else None), pe.route.dz_blocks
            epi = L.ConvEpilogue(L.ptr(pe.Y), coef, act, node.pad, self.mode, s0.H, s0.W, L.ptr(pe.dz_part), blocks,
                                 int(self.mc_dtype == L.MC_MIX16))
            self._probe_begin()
            L.call("mc_conv2d_fused", C.byref(e.ddesc), L.ptr(dY), None, None, L.ptr(e.dbank), None,
                   L.ptr(dxp[0]), None, None, C.byref(epi), st)
            self._probe_end(e.ddesc, "dgrad+dz " + node.name, extra_in=s0.C * s0.H * s0.W)
            L.call("mc_fold_padded_dz", L.ptr(dxp[0]), N, s0.C, s0.H, s0.W, node.pad, self.mode, self.mc_dtype,
                   L.ptr(pe.Y), coef, act, L.ptr(pe.dz_part), blocks, pe.route.dz_tiles, st)
            bk.dz[node.srcs[0]] = L.GradSrc(L.ptr(dxp[0]), L.GSRC_PADFOLD, node.pad, self.mode, 1, s0.H, s0.W)
            return
        self._probe_begin()
        L.call("mc_conv2d", C.byref(e.ddesc), L.ptr(dY), None, L.ptr(e.dbank), None, L.ptr(dxp[0]),
               L.ptr(dxp[1]) if len(dxp) > 1 else None, None, st)
        self._probe_end(e.ddesc, "dgrad " + node.name)
        # adjoint of the padding: fold the halo onto the interior once, consumers read at an offset (the two outputs of
        # a convolution over concatenated sources in one launch)
        live = [(i, s, buf) for i, s, buf in zip(node.srcs, srcs, dxp) if s.requires_grad]
        if len(live) == 2 and (live[0][1].H, live[0][1].W) == (live[1][1].H, live[1][1].W):
            (_, a, abuf), (_, b, bbuf) = live
            L.call("mc_fold_padded2", L.ptr(abuf), a.C, L.ptr(bbuf), b.C, N, a.H, a.W, node.pad, self.mode, self.mc_gdtype, st)
        else:
            for _, s, buf in live:
                L.call("mc_fold_padded", L.ptr(buf), N, s.C, s.H, s.W, node.pad, self.mode, self.mc_gdtype, st)
        for i, s, buf in live:
            bk.srcs[i].append(L.GradSrc(L.ptr(buf), L.GSRC_PADFOLD, node.pad, self.mode, 1, s.H, s.W))

    def _pack_all_banks(self, params, st):
        """Forward and input-gradient banks of every layer in one batched launch per 24 jobs (weights are fixed
        within a step); the eight border banks of every learned-padding layer in one launch per 16 layers."""
        jobs = []        # (a learned layer's main bank: forward as launched (fdesc), gradient of the valid conv)
        for e, fdesc, wname in ([(e, e.desc, "weight") for e in self.convs] + [(e, e.fdesc, "conv.weight") for e in self.learned]):
            w = L.ptr(self._param(params, e.node.name + wname))
            jobs.append((fdesc, w, 0, L.ptr(e.bank)))
            if e.need_dgrad:
                jobs.append((e.desc, w, 1, L.ptr(e.dbank)))
        if jobs:
            L.call("mc_pack_weights_batched", *_columns(jobs, L.ConvDesc, C.c_void_p, C.c_int32, C.c_void_p), len(jobs), st)
        n = len(self.learned)
        if n:
            descs, fw, dg = _columns([(e.ldesc, L.ptr(e.lbank), L.ptr(e.ldbank)) for e in self.learned],
                                     L.LearnedDesc, C.c_void_p, C.c_void_p)
            ws = (C.c_void_p * (8 * n))(*[L.ptr(self._param(params, e.node.name + b + ".weight"))
                                          for e in self.learned for b in L.LEARNED_FRAME_BANKS])
            L.call("mc_learned_pack_banks_batched", descs, ws, fw, dg, n, st)

    # -------------------------------------------------------------- measurement hooks (bench.py)
    def enable_probe(self, passes: int = 3):
        """Record a HIP-event pair (on the launch stream) around every mc_conv2d launch.  The timing events are created and
        recorded once up front: creating them lazily stalled the host for ~80 ms when the runtime grew its signal pool in the
        middle of a pass, and that stall landed inside one event pair (round 2: a 7 ms "launch" of a 50 us kernel)."""
        self._probe = []
        n = 2 * (2 * len(self.convs) + 8) * max(passes, 1)
        self._probe_pool = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
        for ev in self._probe_pool:
            ev.record()
        torch.cuda.synchronize()
        return self._probe

    def disable_probe(self):
        self._probe = None
        self._probe_pool = []

    def _probe_event(self):
        ev = self._probe_pool.pop() if self._probe_pool else torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def _probe_begin(self):
        if self._probe is not None:
            self._probe_ev = self._probe_event()

    def _probe_end(self, d, label, extra_in=0):
        """extra_in: further algorithmic input elements per sample (the producer's y an epilogue-fused launch reads once)."""
        if self._probe is not None:
            ev = self._probe_event()
            es = torch.tensor([], dtype=self.t_dtype).element_size()       # (forward and gradient tensors have the same width)
            ho, wo = d.h + 2 * d.pad - d.k + 1, d.w + 2 * d.pad - d.k + 1
            cin = d.c_in0 + d.c_in1
            nbytes = d.n * es * (cin * d.h * d.w + d.c_out * ho * wo + extra_in)   # algorithmic: read inputs once, write output once
            flops = 2.0 * d.n * cin * d.c_out * d.k * d.k * ho * wo
            name = L.load().mc_conv_kernel_name(C.byref(d)).decode()
            shape = f"{label.split()[0]} {cin}->{d.c_out} k{d.k} {d.n}x{d.h}x{d.w}"
            self._probe.append((name, shape, self._probe_ev, ev, nbytes, flops))

    @staticmethod
    def kernel_family(name):
        """k_conv_rr_bf16<5,f32out> -> k_conv_rr_bf16<5>: every instantiation of a kernel for one filter size is ONE family
        (forward f16 / input gradient bf16 / dz epilogue / f32 output differ in a few instructions of the same schedule)."""
        return name.split(",")[0].rstrip(">") + ">"

    @staticmethod
    def probe_summary(probe, hbm_peak_gbs):
        """Dominant conv kernel FAMILY (largest total time): algorithmic bytes per launch / mean launch duration over ALL its
        launches of a step -- the same set of launches bench.py's `traffic` figure is weighted over."""
        probe = [(Engine.kernel_family(name), *rest) for name, *rest in probe]
        groups = {}
        for name, label, e0, e1, nbytes, flops in probe:
            g = groups.setdefault(name, dict(ms=0.0, bytes=0.0, flops=0.0, n=0))
            g["ms"] += e0.elapsed_time(e1)
            g["bytes"] += nbytes
            g["flops"] += flops
            g["n"] += 1
        if not groups:                               # (a network of learned-padding layers only: no plain mc_conv2d node probed)
            return {"bound": "hbm", "achieved": None, "peak": hbm_peak_gbs, "unit": "GB/s", "frac": None, "traffic": None,
                    "kernel": None, "launches": 0}
        name, g = max(groups.items(), key=lambda kv: kv[1]["ms"])
        ach = g["bytes"] / (g["ms"] * 1e-3) / 1e9
        # the same kernel serves every level of the network: its launches by layer shape (the five that take the most time)
        shapes = {}
        for nm, shape, e0, e1, nbytes, flops in probe:
            if nm == name:
                v = shapes.setdefault(shape, dict(ms=0.0, bytes=0.0, n=0))
                v["ms"] += e0.elapsed_time(e1)
                v["bytes"] += nbytes
                v["n"] += 1
        by_shape = [{"layer": k, "launches": v["n"], "avg_launch_us": 1e3 * v["ms"] / v["n"],
                     "achieved": v["bytes"] / (v["ms"] * 1e-3) / 1e9, "frac": v["bytes"] / (v["ms"] * 1e-3) / 1e9 / hbm_peak_gbs}
                    for k, v in sorted(shapes.items(), key=lambda kv: -kv[1]["ms"])[:5]]
        return {"bound": "hbm", "achieved": ach, "peak": hbm_peak_gbs, "unit": "GB/s", "frac": ach / hbm_peak_gbs,
                "traffic": None, "kernel": name, "launches": g["n"], "avg_launch_us": 1e3 * g["ms"] / g["n"],
                "avg_algorithmic_MB_per_launch": g["bytes"] / g["n"] / 1e6,
                "tflops": g["flops"] / (g["ms"] * 1e-3) / 1e12,
                "share_of_conv_time": g["ms"] / sum(v["ms"] for v in groups.values()), "by_shape": by_shape}

    def algorithmic_bytes_per_sample(self, precision=None) -> float:
        """3 s (sum_in + sum_out over the conv layers) + s_io (C_i + 2 C_o) H W."""
        s = 2 if (precision or self.precision) in ("bf16", "mixed") else 4
        tot = 0
        for e in self.learned + self.spectral:      # (a spectral layer reads its input once and writes its output once)
            src, o = self.T[e.node.srcs[0]], self.T[e.node.out]
            tot += src.C * src.H * src.W + o.C * o.H * o.W
        for d in (e.desc for e in self.convs):
            ho, wo = d.h + 2 * d.pad - d.k + 1, d.w + 2 * d.pad - d.k + 1
            tot += (d.c_in0 + d.c_in1) * d.h * d.w + d.c_out * ho * wo
        # (s_io = s: SURVEY §8d prices the boundary tensors in the storage type as well; round 2 used 4 bytes here, which
        # flattered hbm_roofline_frac_step by 1.7 %)
        return 3.0 * s * tot + float(s) * (self.g.c_in + 2 * self.g.c_out) * self.out_h * self.out_w

    def activation_bytes(self) -> int:
        tot = 0
        for e in self.plan:
            for b in (getattr(e, "Y", None), getattr(e, "dsrc", None), *getattr(e, "dxp", ())):
                if b is not None:
                    tot += b.numel() * b.element_size()
        for t in self.T.values():
            if t.buf is not None:
                tot += t.buf.numel() * t.buf.element_size()
        return tot
