"""Host-side launch recorder of the loss and of the curl heads: the counterpart of tests/engine_trace.py for `StokesLoss` and
the three autograd functions of pytorch_networks_convae.py.  No GPU.

`engine_trace.host_stubs` records every `L.call` (the host query mc_loss_fused_blocks still reaches the library); the tensors
are CPU tensors, so the `.zero_()` calls of the loss, which are torch operations and no library calls, do run: `trace_loss`
fills `gy` and `sums` with a sentinel between its two evaluations and says in two extra entries of the second trace whether
each was zeroed.

Run as a script it dumps the traces of the configuration table (`table()`) as JSON:

    python tests/loss_trace.py traces.json

It imports whichever `pbml_mantle_convection_amd` comes first on sys.path (this tree's when none does), so the same file run
against two checkouts gives two files to compare.
"""
import contextlib
import json
import os
import sys

import torch

import engine_trace as ET

N, H, W = 2, 9, 70
CROP = 3
SENTINEL = 7.0


def _losses():
    ET._modules()
    from pbml_mantle_convection_amd import losses
    return losses


@contextlib.contextmanager
def fused_loss(on):
    """`losses.FUSED_LOSS` = on for the block (None: as it is)."""
    losses = _losses()
    old = losses.FUSED_LOSS
    if on is not None:
        losses.FUSED_LOSS = bool(on)
    try:
        yield losses
    finally:
        losses.FUSED_LOSS = old


def truth_channels(loss):
    return (3 if loss.p_pred else 2) + (1 if loss.has_T else 0)


def loss_inputs(loss, N, Cc, H, W, cb8=False, make=torch.zeros):
    """The arguments of `loss.evaluate` at a shape: (positional, keyword), every tensor f32 and contiguous (so that evaluate
    passes them on as they are and a trace names the same buffers in both evaluations)."""
    g = 2 if loss.curl_valid else 0
    y = make((N, Cc, H + g, W + g))
    kw = {}
    if cb8:
        kw["cb8"] = (make((N, (Cc + 7) // 8, H, W + 2 * CROP, 8)), make((N, Cc)), CROP, (N, Cc, H, W))
    mom = (make((N, H, W)), make((N, 3)), make((N,))) if loss.lambda_mom != 0.0 else (None, None, None)
    if loss.advect_cn is not None:
        kw["advect"] = (make((N, 7, H, W)), make((N,)))
    return (None if cb8 else y, make((N, truth_channels(loss), H, W)), *mom), kw


def trace_loss(loss, N, Cc, H, W, cb8=False):
    """Two evaluations of `loss` on CPU tensors: dict(first=, second= the normalised (entry, arguments) lists, labels= the
    pointer labels of the planes of y and gy, "y+k" / "gy+k" -> label or None where no launch names that plane).  `second`
    ends with ("gy.zero_", [zeroed]) and ("sums.zero_", [zeroed])."""
    args, kw = loss_inputs(loss, N, Cc, H, W, cb8)
    out = {}
    with ET.host_stubs() as rec:
        for which in ("first", "second"):
            rec.reset()
            if which == "second":
                loss.gy.fill_(SENTINEL)
                loss.sums.fill_(SENTINEL)
            loss.evaluate(*args, **kw)
            out[which] = list(rec.entries)
        out["second"] += [("gy.zero_", [bool((loss.gy == 0).all())]), ("sums.zero_", [bool((loss.sums == 0).all())])]
        plane = 4 * loss.gy.shape[2] * loss.gy.shape[3]
        out["labels"] = {}
        for name, t in (("y", args[0]), ("gy", loss.gy)):
            for k in range(Cc if t is not None else 0):
                out["labels"][f"{name}+{k}"] = rec.labels.get(t.data_ptr() + k * plane)
    return out


def trace_head(fn, y_shape, blurr=None):
    """One forward and backward of the autograd function `fn` (its class name in pytorch_networks_convae.py) on a CPU tensor:
    the normalised (entry, arguments) list.  blurr: None for a function without the argument."""
    ET._modules()
    from pbml_mantle_convection_amd import pytorch_networks_convae as P
    y = torch.zeros(y_shape, requires_grad=True)
    with ET.host_stubs() as rec:
        outs = getattr(P, fn).apply(y, 10.0, *(() if blurr is None else (blurr,)))
        sum(o.sum() for o in outs).backward()
        return list(rec.entries)


def _row(Cc=None, fused=None, cb8=False, **kw):
    return dict(kw=kw, Cc=Cc, fused=fused, cb8=cb8)


def _variations(t, name, **base):
    """The four variations every family carries: a spare output channel (the zeroing rule), the scaled loss (mc_loss_minmax),
    the squared norm, and no gradient through the temperature term."""
    t[name + " spare channel"] = _row(Cc="+1", **base)
    t[name + " loss_scale"] = _row(loss_scale=True, **base)
    t[name + " l2"] = _row(norm="l2", **base)
    t[name + " t_grad off"] = _row(t_grad=False, **base)


def table():
    """name -> dict(kw= keyword arguments of StokesLoss, Cc= output channels (None: channels_needed(), "+1": one more), fused=
    the value of losses.FUSED_LOSS the loss is built and run under, cb8= the CB8 form): the configurations on which a change to
    the loss is compared launch for launch with its parent, at N = 2, H x W = 9 x 70."""
    t = {}
    for lt in ("mae", "mass"):
        for p in (False, True):
            for lam in (0.0, 1e-6):
                kw = dict(p_pred=p, loss_type=lt, lambda_mom=lam)
                t[f"unet {lt} p{int(p)} lam{lam:g} fused"] = _row(fused=True, **kw)
                t[f"unet {lt} p{int(p)} lam{lam:g} cb8"] = _row(fused=True, cb8=True, **kw)
                t[f"unet {lt} p{int(p)} lam{lam:g} split"] = _row(fused=False, **kw)
    for p in (False, True):
        for lam in (0.0, 1e-6):
            t[f"unet curl p{int(p)} lam{lam:g}"] = _row(p_pred=p, loss_type="curl", lambda_mom=lam)
    for lt in ("mae", "mass", "curl"):
        for p in (False, True):
            for cn in (None, 2e4):
                for blurr in ((False, True) if lt == "curl" else (False,)):
                    t[f"newfluidnet {lt} p{int(p)} ad{int(cn is not None)} blurr{int(blurr)}"] = _row(
                        p_pred=p, loss_type=lt, has_T=False, advect_cn=cn, blurr=blurr)
    for blurr in (False, True):
        for cn in (None, 2e4):
            t[f"fluidnet ad{int(cn is not None)} blurr{int(blurr)}"] = _row(
                p_pred=False, loss_type="curl", has_T=False, curl_valid=True, advect_cn=cn, blurr=blurr)
    _variations(t, "unet mass fused", fused=True, p_pred=True, loss_type="mass", lambda_mom=1e-6)
    _variations(t, "unet mass cb8", fused=True, cb8=True, p_pred=True, loss_type="mass", lambda_mom=1e-6)
    _variations(t, "unet mass split", fused=False, p_pred=True, loss_type="mass", lambda_mom=1e-6)
    _variations(t, "unet curl", p_pred=True, loss_type="curl", lambda_mom=1e-6)
    _variations(t, "newfluidnet mass", p_pred=True, loss_type="mass", has_T=False, advect_cn=2e4)
    _variations(t, "newfluidnet curl", p_pred=True, loss_type="curl", has_T=False, advect_cn=2e4, blurr=True)
    _variations(t, "fluidnet", p_pred=False, loss_type="curl", has_T=False, curl_valid=True, advect_cn=2e4, blurr=True)
    return t


def head_table():
    """name -> (autograd function, shape of y, blurr or None)."""
    t = {"_CurlHead": ("_CurlHead", (N, 3, H, W), None)}
    for b in (False, True):
        t[f"_CurlUV blurr{int(b)}"] = ("_CurlUV", (N, 2, H, W), b)
        t[f"_CurlValid blurr{int(b)}"] = ("_CurlValid", (N, 1, H + 2, W + 2), b)
    return t


def build(row):
    """(loss, Cc) of a row of `table()`; call it, and trace the loss, inside `fused_loss(row["fused"])`."""
    loss = _losses().StokesLoss(**row["kw"])
    Cc = loss.channels_needed() + (1 if row["Cc"] == "+1" else 0)
    return loss, Cc


def trace_row(row):
    with fused_loss(row["fused"]):
        loss, Cc = build(row)
        return trace_loss(loss, N, Cc, H, W, cb8=row["cb8"])


def dump(path):
    out = {name: trace_row(row) for name, row in table().items()}
    out.update({name: trace_head(*row) for name, row in head_table().items()})
    with open(path, "w") as f:
        json.dump(out, f)
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tests/loss_trace.py OUT.json")
    res = dump(sys.argv[1])
    print(f"{len(res)} traces of {os.path.abspath(_losses().__file__)}")
