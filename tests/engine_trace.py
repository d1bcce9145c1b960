"""Host-side launch recorder of the engine: one forward + backward of an `Engine` on CPU tensors, with every launch recorded
instead of issued.  No GPU.

Four stubs make that possible: `L.call` records (the host queries in `L.VALUE_RETURNING` still reach the library), `L.stream`
and `L.require_cuda` do nothing, `Engine._param` hands the parameter over unchecked.  A trace is a list of
(entry name, normalised arguments): numbers as they are, device pointers as small integer labels in order of first appearance
(NULL = None), `byref` structs field by field, ctypes arrays as lists -- so two source trees give equal traces exactly when
they pass the same buffers in the same places of the same launches.

Run as a script it dumps the traces of the configuration table (`table()`) as JSON:

    python tests/engine_trace.py traces.json

It imports whichever `pbml_mantle_convection_amd` comes first on sys.path (this tree's when none does), so the same file
run against two checkouts gives two files to compare.
"""
import contextlib
import ctypes as C
import json
import os
import sys

import torch

HEADLINE = (2, 128, 506)


def _modules():
    try:
        import pbml_mantle_convection_amd  # noqa: F401
    except ImportError:
        sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd import engine as E
    return L, E


class Recorder:
    def __init__(self, L):
        self.L, self.entries, self.labels = L, [], {}

    def reset(self):
        self.entries, self.labels = [], {}

    def _label(self, p):
        p = getattr(p, "value", p)
        if not p:
            return None
        return self.labels.setdefault(int(p), len(self.labels) + 1)

    def _struct(self, s):
        return {n: (self._label(getattr(s, n)) if t is C.c_void_p else getattr(s, n)) for n, t in s._fields_}

    def _arg(self, a, argtype):
        a = getattr(a, "_obj", a)                            # byref(x) -> x
        if isinstance(a, C.Structure):
            return self._struct(a)
        if isinstance(a, C.Array):
            if issubclass(a._type_, C.Structure):
                return [self._struct(s) for s in a]
            return [self._label(v) for v in a] if a._type_ is C.c_void_p else list(a)
        if argtype is C.c_void_p or a is None:
            return self._label(a)
        return a

    def call(self, name, *args):
        if name in self.L.VALUE_RETURNING:
            return getattr(self.L.load(), name)(*args)
        types = self.L.SIGNATURES[name][1]
        assert len(types) == len(args), f"{name}: {len(args)} arguments for {len(types)} parameters"
        self.entries.append((name, [self._arg(a, t) for a, t in zip(args, types)]))
        return 0


@contextlib.contextmanager
def host_stubs():
    """Installs the four stubs; yields the Recorder."""
    L, E = _modules()
    rec = Recorder(L)
    saved = (L.call, L.stream, L.require_cuda, E.Engine.__dict__["_param"])
    L.call, L.stream, L.require_cuda = rec.call, (lambda: None), (lambda t, name="tensor": None)
    E.Engine._param = staticmethod(lambda params, name: params[name])
    try:
        yield rec
    finally:
        L.call, L.stream, L.require_cuda = saved[:3]
        E.Engine._param = saved[3]


def make_engine(graph, precision, env=None):
    """An Engine built under the given MANTLE_* settings (the switches are read in the constructor)."""
    _, E = _modules()
    env = {k: str(v) for k, v in (env or {}).items()}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return E.Engine(graph, precision)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def param_names(graph):
    L, E = _modules()
    names = []
    for n in graph.nodes:
        if n.kind != "conv":
            continue
        if n.spectral:
            names += [n.name + "weights1", n.name + "weights2"]
        elif n.learned:
            names += [n.name + b + ".weight" for b in E.BANKS] + [n.name + "learnable_bias"]
        else:
            names += [n.name + "weight", n.name + "bias"]
        if n.gn_name:
            names += [n.gn_name + "weight", n.gn_name + "bias"]
    return names


def trace_step(eng, shape, drop=False, unpack=True, gsum=False, steps=1):
    """The traces of `steps` consecutive forward + backward calls of `eng` at input shape (N, H, W): a list of
    (forward entries, backward entries), labels counted from 1 within each step."""
    N, H, W = shape
    g = eng.g
    cpu = torch.device("cpu")
    params = {n: torch.zeros(1) for n in param_names(g)}
    grads = {n: torch.zeros(1) for n in params}
    x = torch.zeros((N, g.c_in, H, W))
    out = []
    with host_stubs() as rec:
        eng.configure(N, H, W, cpu)
        gout = torch.zeros((N, g.c_out, eng.out_h, eng.out_w))
        blocks = 3
        gs = (torch.zeros((N, blocks, 4)), blocks) if gsum else None
        for _ in range(steps):
            rec.reset()
            eng.forward(x, params, drop=drop, unpack=unpack)
            nf = len(rec.entries)
            eng.backward(gout, params, grads, gsum=gs)
            out.append((rec.entries[:nf], rec.entries[nf:]))
    return out


FUSE3 = {"MANTLE_FUSE": 3, "MANTLE_FUSE_MAXPIX": 1073741824}
SWITCHES = {"dz_rr0": {"MANTLE_FUSE_DZ_RR": 0}, "wgrad_dz0": {"MANTLE_WGRAD_DZ": 0}, "gn_small0": {"MANTLE_GN_SMALL_PIX": 0},
            "fuse3": FUSE3, "fuse1": {"MANTLE_FUSE": 1}, "fuse2": {"MANTLE_FUSE": 2}}
PRECISIONS = ("fp32", "bf16", "mixed")


def headline(r_p="reflect", levels=5, c_h=16, c_o=4, use_symm=True):
    _, E = _modules()
    return E.unet_graph(levels, 10, c_h, c_o, act="gelu", r_p=r_p, use_symm=use_symm, repeats=3, f=5)


def table():
    """name -> (graph, shape, precisions, env, keyword arguments of trace_step): the configurations on which a change to the
    engine is compared launch for launch with its parent."""
    L, E = _modules()
    kw = dict(act="gelu", use_symm=True, f=5)
    small, layer = (2, 64, 96), (2, 40, 54)

    def row(g, shape=HEADLINE, env=None, precisions=PRECISIONS, **step):
        return g, shape, precisions, env, step
    t = {"unet": row(headline()), "unet gsum": row(headline(), gsum=True), "unet cb8 output": row(headline(), unpack=False)}
    for r_p in ("zeros", "replicate"):
        t["unet " + r_p] = row(headline(r_p))
    for name, env in SWITCHES.items():
        t["unet " + name] = row(headline(), env=env)
    t["unet relu fuse3"] = row(E.unet_graph(5, 10, 16, 4, act="relu", r_p="reflect", use_symm=True, repeats=3, f=5), env=FUSE3,
                               precisions=("mixed",))
    for r_p in ("reflect", "learned"):                      # concat nodes with gathered operands
        t["unet6 " + r_p] = row(headline(r_p, c_h=6, c_o=2, use_symm=False))
    t["unet3 learned"] = row(E.unet_graph(3, 10, 8, 4, r_p="learned", repeats=2, **kw), (2, 48, 70))
    t["unet2"] = row(headline(levels=2), (2, 40, 150))
    for loss in ("mae", "curl"):
        t["convae " + loss] = row(E.convae_graph(2, 3, 16, 3, act="gelu", r_p="reflect", use_symm=True, repeats=2, f=3, loss_type=loss),
                                  (2, 64, 48))
    for name, fn in (("newfluidnet", E.newfluidnet_graph), ("fluidnet", E.fluidnet_graph)):
        t[name + " learned"] = row(fn(3, 7, 16, 4, r_p="learned", repeats=2, **kw), small)
        t[name + " spectral"] = row(fn(3, 7, 16, 4, r_p="zeros", repeats=2, spectral=True, **kw), small)
        t[name + " reflect"] = row(fn(3, 7, 16, 4, r_p="reflect", repeats=2, **kw), small)
        t[name + " reflect fuse3"] = row(fn(3, 7, 16, 4, r_p="reflect", repeats=2, **kw), small, FUSE3)
        for r_p in ("learned", "reflect"):
            g = fn(3, 7, 16, 4, r_p=r_p, repeats=2, drop_rate=0.25, **kw)
            t[f"{name} drop {r_p}"] = row(g, small, drop=True)
            t[f"{name} drop {r_p} fuse3"] = row(g, small, FUSE3, drop=True)
        t[name + " drop off"] = row(g, small, precisions=("mixed",))       # a dropout graph in evaluation mode
    gn = (L.POST_GN_ACT, "gelu", 4, True)
    t["layer sym"] = row(E.single_layer_graph(10, 16, 5, 2, "reflect", 4, *gn), layer)
    t["layer sym act"] = row(E.single_layer_graph(10, 16, 5, 2, "zeros", 4, L.POST_ACT, "gelu", 1, False), layer)
    t["layer sym drop"] = row(E.single_layer_graph(10, 16, 5, 2, "zeros", 4, *gn, drop_rate=0.25), (2, 80, 90), drop=True)
    t["layer learned dx"] = row(E.single_layer_graph(10, 16, 5, 2, "zeros", 4, *gn, learned=True, bc_x=4, input_grad=True), layer)
    t["layer spectral dx"] = row(E.single_layer_graph(6, 12, 0, 0, "zeros", 0, L.POST_GN_ACT, "tanh", 3, True, spectral=True,
                                                      input_grad=True), layer)
    return t


def dump(path):
    out = {}
    for name, (g, shape, precisions, env, kw) in table().items():
        for prec in precisions:
            eng = make_engine(g, prec, env)
            (fwd, bwd), = trace_step(eng, shape, **kw)
            out[f"{name} / {prec}"] = {"forward": fwd, "backward": bwd}
    with open(path, "w") as f:
        json.dump(out, f)
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tests/engine_trace.py OUT.json")
    res = dump(sys.argv[1])
    _, E = _modules()
    print(f"{len(res)} traces of {os.path.abspath(E.__file__)}")
    for k in ("unet / fp32", "unet / bf16", "unet / mixed"):
        print(k, len(res[k]["forward"]), "forward,", len(res[k]["backward"]), "backward entries")
