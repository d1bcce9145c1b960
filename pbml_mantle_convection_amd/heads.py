"""The curl heads -- u, v as centred differences of a streamfunction channel -- and the one place that launches them
(libmantle_hip: mc_curl_head_* / mc_curl_valid_* and, with `-blurr 1`, their mc_curl_blur_* twins).  The autograd functions
of pytorch_networks_convae.py, Trainer._roll_chain and StokesLoss all go through `CurlHead`."""
from __future__ import annotations

import enum
from dataclasses import dataclass

from . import _lib as L


class HeadForm(enum.Enum):
    WALL_T = "wall_t"      # Unet (reference pytorch_networks_convae.py:2038-2070): antisymmetric walls, zero corners; T = channel 1
    WALL = "wall"          # NewFluidNet (:1360-1388): the same walls, no T channel
    VALID = "valid"        # FluidNet (:1681-1697): plain differences of a grown (H+2) x (W+2) field, no wall fix-up


T_CLIP = (0.0, 1.5)
BLURR_NEEDS_FLUIDNET = ("blurr is the streamfunction blur of NewFluidNet / FluidNet: loss_type 'curl' and has_T = False (the "
                        "Unet's blurr, a randomly drawn Gaussian, is not built)")
# (form, blurr) -> (forward, backward); blurr: of the streamfunction's 3 x 3 box mean, inside the same launches
ENTRIES = {
    (HeadForm.WALL_T, False): ("mc_curl_head_fwd", "mc_curl_head_bwd"),
    (HeadForm.WALL, False): ("mc_curl_head_fwd", "mc_curl_head_bwd"),
    (HeadForm.WALL, True): ("mc_curl_blur_head_fwd", "mc_curl_blur_head_bwd"),
    (HeadForm.VALID, False): ("mc_curl_valid_fwd", "mc_curl_valid_bwd"),
    (HeadForm.VALID, True): ("mc_curl_blur_valid_fwd", "mc_curl_blur_valid_bwd"),
}


@dataclass(frozen=True, slots=True)
class CurlHead:
    """Pointers are device addresses (None = NULL), strides are batch strides in floats, H x W is the grid of u and v."""
    form: HeadForm
    blurr: bool = False
    a_bound: float = 10.0

    def __post_init__(self):
        if (self.form, self.blurr) not in ENTRIES:
            raise ValueError(BLURR_NEEDS_FLUIDNET)

    def out_hw(self, Hy, Wy):
        """The grid of u, v for a network output of Hy x Wy."""
        return (Hy - 2, Wy - 2) if self.form is HeadForm.VALID else (Hy, Wy)

    def ws_floats(self, N, H, W):
        """Floats of workspace `backward` needs."""
        return 0 if self.form is HeadForm.VALID else 2 * N * (H - 2) * (W - 2)

    def _t_plane(self, HW):
        """(byte offset of the T plane, channel 1, in y and in its gradient; t_lo; t_hi) of a wall form."""
        return (4 * HW, *T_CLIP) if self.form is HeadForm.WALL_T else (None, 0.0, 0.0)

    def forward(self, y_ptr, y_stride, N, H, W, u, v, t_out=None, stream=None):
        """u, v [N, H, W] (and t_out, the clipped T, with WALL_T) from channel 0 (and 1) of y."""
        fwd = ENTRIES[self.form, self.blurr][0]
        if self.form is HeadForm.VALID:
            return L.call(fwd, y_ptr, N, H, W, y_stride, self.a_bound, u, v, stream)
        t_off, lo, hi = self._t_plane(H * W)
        t_in = None if t_off is None else y_ptr + t_off
        return L.call(fwd, y_ptr, t_in, N, H, W, y_stride, self.a_bound, lo, hi, u, v, t_out, stream)

    def backward(self, gu, gv, gt, y_ptr, y_stride, N, H, W, ga_ptr, g_stride, ws, stream=None):
        """The adjoint into channel 0 (and 1) of the gradient at ga_ptr; ws: `ws_floats` floats."""
        bwd = ENTRIES[self.form, self.blurr][1]
        if self.form is HeadForm.VALID:
            return L.call(bwd, gu, gv, N, H, W, self.a_bound, ga_ptr, g_stride, stream)
        t_off, lo, hi = self._t_plane(H * W)
        t_in, gt_in = (None, None) if t_off is None else (y_ptr + t_off, ga_ptr + t_off)
        return L.call(bwd, gu, gv, gt, t_in, N, H, W, self.a_bound, lo, hi, ga_ptr, gt_in, y_stride, g_stride, ws, stream)

