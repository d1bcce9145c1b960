"""BoundaryLearnedConvolution2D — the reference's "learned padding" layer (pytorch_networks_convae.py:802-1065; SURVEY.md
§8(f) row N4) on the HIP path: nine bias-free VALID convolutions (one on the whole input, eight on the border strips of
width k + 1 / k) framed together, plus one shared bias.

Stand-alone, the layer is a one-node graph on the engine (engine.single_layer_graph(learned=True, input_grad=True)), as
SymmetricConv2d and FluidLayer are: Engine._plan_learned / _fwd_learned / _bwd_learned are the only executor of
the layer, inside a network or alone.  The main bank runs on the library's conv kernels (`mc_conv2d`, `mc_conv2d_wgrad*`)
as a zero-padded 'same' convolution straight into the output (its interior is the valid result); the frame of the eight
border banks -- forward, filter gradient and input gradient -- is one `mc_learned_frame_*` launch per direction that reads
the input / the output gradient in place.  As in the reference, the strip cut from the LAST rows lands in the FIRST output
rows and vice versa (:1057-1060).  The gradient w.r.t. the input comes back through the autograd bridge (hipnet).

What the stand-alone module shares with every other HipNetMixin layer: set_precision takes 'fp32', 'bf16' and 'mixed';
there is one configured shape per precision (a forward at another N x H x W re-plans); the output gradient is packed by
mc_pack_grad_nchw, the main bank's filter gradient is combined by mc_conv2d_wgrad_finalize_batched with the other layers'
(here: alone), and the shared bias takes the frame's share before the interior's.  Only bc_x = bc_y = 1 (output size =
input size) is implemented for the stand-alone module: the graph is built for it; the engine's learned node takes any bc.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from .engine import BANKS, fluid_sym_h, single_layer_graph
from .hipnet import HipNetMixin
from .symmetric_layers_torch import SymmetricConv2d


class BoundaryLearnedConvolution2D(nn.Module, HipNetMixin):
    """Same constructor, sub-modules and state_dict keys as the reference (nine `nn.Conv2d` / `SymmetricConv2d` banks with
    bias=False and 'valid' padding, `learnable_bias` [1, c_o, 1, 1]); these names are the engine's parameter names of the
    node "" (SymmetricConv2d(bias=False) exposes its unique filters as `.weight`)."""

    def __init__(self, c_i, c_o, k, stride=1, use_symm=False):
        super().__init__()
        if k not in (3, 5) or stride != 1:
            raise NotImplementedError("HIP BoundaryLearnedConvolution2D supports 3x3 / 5x5 kernels, stride 1")
        self.c_i, self.c_o, self.k, self.use_symm = c_i, c_o, k, use_symm
        h_s = fluid_sym_h(c_o) if use_symm else 0
        for name in BANKS:
            if use_symm:
                mod = SymmetricConv2d(c_i, c_o, k, bias=False, padding="valid", symmetry={"h": h_s, "v": 0, "hv": 0})
            else:
                mod = nn.Conv2d(in_channels=c_i, out_channels=c_o, kernel_size=k, padding="valid", bias=False)
            setattr(self, name, mod)
        self.learnable_bias = nn.Parameter(torch.zeros(1, c_o, 1, 1))
        self._init_hipnet(single_layer_graph(c_i, c_o, k, k // 2, "zeros", h_s, L.POST_NONE, "none", 1, gn=False, learned=True,
                                             input_grad=True))

    def forward(self, x, bc_x=1, bc_y=1):
        if bc_x != 1 or bc_y != 1:
            raise NotImplementedError("bc_x / bc_y > 1 (field-growing strips of the Unet's first layer) are not implemented")
        return self._run_graph(x)
