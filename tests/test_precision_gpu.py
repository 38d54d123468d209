"""Every matrix-core family against float64: the bf16x3 claim (six MFMA terms of an exact three-way split, fp32
accumulation) measured on the device.

Errors are row-normalised (tests/precision.py: rel_err_rows, one output channel of one image per row) and bounded by
precision.x3_bound of the k chain the kernel runs (for chains of at most 256, the bound tests/test_precision.py shows to
lie between the six-term product and one that lost a 2^-16 term; longer chains are bounded by their accumulation error).
Each family is forced through the tuning knobs the kernel tests use, the knobs are reset on leaving the `knobs` scope,
and the plan queries confirm the family actually served the call.  Inputs: uniform(-1, 1) and mixed scales (activations
per input channel over 2^-10 .. 2^10, weights per output row over 2^-12 .. 1; for weight gradients the input scales lie
along the contracted pixels).

Composite operations (LayerNorm on load, softmax attention, the GELU gate) are held to at most 2x the error of the same
computation in PyTorch fp32 on the CPU, with a floor of 1e-6.
Run with -s to print the measured errors; the largest per family are in the `measured` table printed at the end.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from promptir_amd import weights as W
from tests import precision as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED = {}      # family -> largest error seen, printed by the last test


def _note(family, err, bound):
    print("%-40s err %.3e  bound %.3e" % (family, err, bound))
    MEASURED[family] = max(MEASURED.get(family, 0.0), err)
    assert err <= bound, (family, err, bound)


def rnd(name, *shape, seed=0):
    return torch.from_numpy((W.uniform01(name, int(np.prod(shape)), seed).reshape(shape) * 2 - 1).astype(np.float32))


def _scaled(t, name, dim, rng):
    """t scaled along `dim` by power-of-two factors over 2^rng[0] .. 2^rng[1]."""
    s = P.mixed_scales(name, t.shape[dim], *rng)
    shape = [1] * t.dim()
    shape[dim] = -1
    return t * s.view(shape)


def _lib():
    from promptir_amd import _lib
    return _lib.lib


DEFAULTS = {4: -1, 20: -1, 24: -1, 25: -1, 26: -1, 43: 45, 44: 1, 45: 1}


class knobs:
    def __init__(self, **kv):
        self.kv = {int(k[1:]): v for k, v in kv.items()}

    def __enter__(self):
        L = _lib()
        for k, v in self.kv.items():
            assert L.pir_tune_set(k, v) == 0, (k, v)

    def __exit__(self, *exc):
        L = _lib()
        for k in self.kv:
            L.pir_tune_set(k, DEFAULTS[k])
        return False


# ---------------------------------------------------------------------------------------------- 1x1 convolutions
FAMILIES_1X1 = {
    "tiled": dict(k20=0, k24=0, k26=0, k43=0, k45=0),
    "tiles32x128": dict(k20=0, k24=0, k26=0, k43=100, k45=0),
    "split_k": dict(k20=0, k24=0, k26=0, k45=1),
    "resident": dict(k20=1, k24=0, k26=0),
    "bstationary": dict(k20=1, k24=1, k26=0),
    "cstationary": dict(k26=1),
}


def _nn_desc(M, K, N, B, dgrad, wd, x, y, r=None):
    from promptir_amd import _lib as LL, ops

    a3, kp = ops._split_weight(wd, dgrad=dgrad)
    g = LL.GemmNN()
    g.M, g.K, g.N, g.O1, g.O2, g.ldx, g.ldy, g.A3, g.a3_kp = M, K, N, B, 1, N, N, a3.data_ptr(), kp
    g.x_s1, g.y_s1 = K * N, M * N
    g.X, g.Y = x.data_ptr(), y.data_ptr()
    if r is not None:
        g.R, g.r_s1, g.ldr = r.data_ptr(), M * N, N
    return g


def _nn_chain(g):
    """The k chain one accumulator of this call runs: K, or K cut into the split-over-k slices (pir_gemm_nn_ws_floats =
    splits x images x M x N)."""
    ws = _lib().pir_gemm_nn_ws_floats(ctypes.byref(g))
    sp = ws // (g.O1 * g.M * g.N) if ws else 1
    return -(-(-(-g.K // 16)) // sp) * 16 if sp > 1 else g.K


def _serves(family, g):
    """Does the forced family serve this call?  (plan: TM*1000 + TN*100 + WM*10 + WN, or 9000 / 9100 / 9200)"""
    L = _lib()
    plan = L.pir_gemm_nn_plan(ctypes.byref(g))
    split = L.pir_gemm_nn_ws_floats(ctypes.byref(g)) > 0
    bm = (plan // 1000) * ((plan // 10) % 10) * 32 if plan < 9000 else 0
    return {"tiled": plan < 9000 and bm in (96, 128) and not split, "tiles32x128": plan < 9000 and bm == 32 and not split,
            "split_k": plan < 9000 and split, "resident": plan == 9000, "bstationary": plan == 9100,
            "cstationary": plan == 9200}[family]


SHAPES_1X1 = [(48, 144, 128), (96, 510, 128), (510, 96, 128), (192, 1020, 32), (384, 2042, 16), (2042, 384, 16)]
_REF_CACHE = {}


def _cols(hw):
    """The pixels the float64 reference is computed on (a 1x1 convolution is per pixel): a stride through the image and
    its last 40 pixels (the tile tails)."""
    return torch.unique(torch.cat([torch.arange(0, hw, 13), torch.arange(max(0, hw - 40), hw)]))


def _case_1x1(cin, cout, side, b, kind):
    key = (cin, cout, side, b, kind)
    if key in _REF_CACHE:
        return _REF_CACHE[key]
    hw = side * side
    x, dy = rnd("x", b, cin, side, side), rnd("dy", b, cout, side, side)
    wf, wd = rnd("w", cout, cin, 1, 1), rnd("wd", cout, cin, 1, 1)
    r = rnd("r", b, cout, side, side)
    if kind == "mixed":
        x, dy = _scaled(x, "x", 1, P.IN_SCALES), _scaled(dy, "dy", 1, P.IN_SCALES)
        wf, wd = _scaled(wf, "wf", 0, P.ROW_SCALES), _scaled(wd, "wd", 1, P.ROW_SCALES)
        r = _scaled(r, "r", 1, P.ROW_SCALES)
    cols = _cols(hw)
    xs = x.reshape(b, cin, hw)[:, :, cols].double()
    dys = dy.reshape(b, cout, hw)[:, :, cols].double()
    y64 = torch.einsum("mk,bkn->bmn", wf.reshape(cout, cin).double(), xs)
    yr64 = y64 + r.reshape(b, cout, hw)[:, :, cols].double()
    dx64 = torch.einsum("mk,bmn->bkn", wd.reshape(cout, cin).double(), dys)
    out = dict(x=x.to(DEV), dy=dy.to(DEV), wf=wf.to(DEV), wd=wd.to(DEV), r=r.to(DEV), cols=cols, y64=y64, yr64=yr64, dx64=dx64)
    _REF_CACHE.clear()
    _REF_CACHE[key] = out
    return out


@pytest.mark.parametrize("kind", ["uniform", "mixed"])
def test_1x1_forward_and_input_gradient_vs_float64(kind):
    """Every family at every model shape it serves (batches 1 and 8): forward, forward + residual epilogue, input gradient."""
    from promptir_amd import ops

    served = {f: 0 for f in FAMILIES_1X1}
    short = {f: 0 for f in FAMILIES_1X1}        # runs at a chain of at most 256, where the bound separates a lost term
    for cin, cout, side in SHAPES_1X1:
        for b in (1, 8):
            c = _case_1x1(cin, cout, side, b, kind)
            hw = side * side
            for family, kn in FAMILIES_1X1.items():
                with knobs(**kn):
                    y = torch.empty(b, cout, side, side, device=DEV)
                    dx = torch.empty(b, cin, side, side, device=DEV)
                    runs = []
                    g = _nn_desc(cout, cin, hw, b, False, c["wf"], c["x"], y)
                    if _serves(family, g):
                        runs.append(("fwd", _nn_chain(g), lambda: ops.conv1x1_forward(c["x"], c["wf"]), c["y64"], cout))
                    g = _nn_desc(cout, cin, hw, b, False, c["wf"], c["x"], y, c["r"])
                    if _serves(family, g):
                        runs.append(("fwd+res", _nn_chain(g), lambda: ops.conv1x1_forward(c["x"], c["wf"], c["r"]), c["yr64"],
                                     cout))
                    g = _nn_desc(cin, cout, hw, b, True, c["wd"], c["dy"], dx)
                    if _serves(family, g):
                        runs.append(("dgrad", _nn_chain(g), lambda: ops.conv1x1_dgrad(c["dy"], c["wd"]), c["dx64"], cin))
                    outs = [(op, chain, call().reshape(b, m, hw)[:, :, c["cols"]], ref) for op, chain, call, ref, m in runs]
                for op, chain, got, ref in outs:
                    _note("1x1 %s %s" % (family, op), P.rel_err_rows(got, ref, (0, 1)), P.x3_bound(chain))
                    served[family] += 1
                    short[family] += chain <= 256
    assert all(short.values()), (served, short)


# ---------------------------------------------------------------------------------------------- 1x1 weight gradients
def _nt_chain(dy, x, b, cout, cin, hw):
    """The k chain of the split-K weight gradient: b*hw pixels cut into `splits` slices (pir_gemm_nt_ws_needed)."""
    from promptir_amd import _lib as LL, ops

    g = LL.GemmNT()
    g.X, g.x_sr, g.ldx = dy.data_ptr(), cout * hw, hw
    g.Y, g.y_sr, g.ldy = x.data_ptr(), cin * hw, hw
    g.M1, g.M2, g.N, g.O1, g.O2, g.BR = cout, cin, hw, 1, 1, b
    splits = max(1, int(ops.lib.pir_gemm_nt_ws_needed(ctypes.byref(g))) // (cout * cin))
    return int(math.ceil(b * hw / splits / 128.0) * 128)


SHAPES_WGRAD = [(48, 144, 128, 1), (96, 510, 128, 1), (192, 1020, 32, 8), (384, 2042, 16, 1), (2042, 384, 16, 1),
                (384, 2042, 16, 8)]


@pytest.mark.parametrize("kind", ["uniform", "mixed"])
def test_1x1_weight_gradient_vs_float64(kind):
    from promptir_amd import ops

    for cin, cout, side, b in SHAPES_WGRAD:
        hw = side * side
        x, dy = rnd("x", b, cin, side, side), rnd("dy", b, cout, side, side)
        if kind == "mixed":     # the contraction runs over the pixels: the "input channel" scales go there, the row scales
            x = _scaled(x.reshape(b, cin, hw), "xp", 2, P.IN_SCALES).reshape(b, cin, side, side)   # on dy's channels
            dy = _scaled(dy, "dy", 1, P.ROW_SCALES)
        xm = x.transpose(0, 1).reshape(cin, b * hw)
        dym = dy.transpose(0, 1).reshape(cout, b * hw)
        ref = dym.double() @ xm.double().t()
        f32_err = P.rel_err_rows(dym @ xm.t(), ref, (0,))
        xd, dyd = x.to(DEV), dy.to(DEV)
        like = torch.empty(cout, cin, 1, 1, device=DEV)
        outs = {}
        for name, kn in (("x3", dict(k25=0)), ("fp32", dict(k25=0, k4=0)), ("xprivate", dict(k25=1))):
            with knobs(**kn):
                chain = min(_nt_chain(dyd, xd, b, cout, cin, hw), b * hw)
                got = ops.conv1x1_wgrad(dyd, xd, like).clone()
            outs[name] = got
            bound = P.x3_bound(min(chain, 4096)) if name != "fp32" else max(2 * f32_err, 1e-6, P.x3_bound(min(chain, 4096)))
            _note("wgrad 1x1 %s" % name, P.rel_err_rows(got.reshape(cout, cin), ref, (0,)), bound)
        assert not torch.equal(outs["x3"], outs["fp32"]), "knob 4 did not change the kernel"


@pytest.mark.parametrize("b", [1, 4])
def test_grouped_low_resolution_weight_gradients_vs_float64(b):
    from promptir_amd import ops

    side, hw = 16, 256
    shapes = [(384, 1152), (384, 384), (384, 2042), (1021, 384)]
    items, refs = [], []
    for k, (cin, cout) in enumerate(shapes):
        x, dy = rnd("gx%d" % k, b, cin, side, side), rnd("gdy%d" % k, b, cout, side, side)
        refs.append(dy.transpose(0, 1).reshape(cout, -1).double() @ x.transpose(0, 1).reshape(cin, -1).double().t())
        items.append((dy.to(DEV), x.to(DEV), torch.empty(cout, cin, 1, 1, device=DEV)))
    with ops.deferred_reductions():
        ops.conv1x1_wgrad_group(items)
    ops.flush_reductions()
    for (dy, x, dw), ref in zip(items, refs):
        _note("wgrad 1x1 grouped", P.rel_err_rows(dw.reshape(ref.shape), ref, (0,)), P.x3_bound(b * hw))


def _ln64(x, g, bta):
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = xd.var(1, keepdim=True, unbiased=False)
    return (xd - mu) / torch.sqrt(var + 1e-5) * g.double().view(1, -1, 1, 1) + bta.double().view(1, -1, 1, 1)


def _ln32(x, g, bta):
    mu = x.mean(1, keepdim=True)
    var = x.var(1, keepdim=True, unbiased=False)
    return (x - mu) / torch.sqrt(var + 1e-5) * g.view(1, -1, 1, 1) + bta.view(1, -1, 1, 1)


LN_SHAPES = [(2, 48, 144, 32, 32), (1, 96, 510, 32, 32), (2, 96, 288, 16, 16)]


@pytest.mark.parametrize("kind", ["uniform", "mixed"])
def test_layernorm_on_load_products_vs_float64(kind):
    """ln_conv1x1_forward (knob 24 = 1), conv1x1_wgrad_ln (knob 25 = 1) and conv1x1_dgrad_ln_backward: LayerNorm
    applied as the operand is loaded / in the store tail, a row-scale epilogue - judged per output row."""
    from promptir_amd import ops

    for b, c, k, h, w in LN_SHAPES:
        hw = h * w
        x = rnd("x", b, c, h, w) * 3 + 0.5
        wt, dy, dres = rnd("w", k, c, 1, 1), rnd("dy", b, k, h, w), rnd("dres", b, c, h, w)
        gam, bet = rnd("g", c) + 1.5, rnd("b", c)
        if kind == "mixed":
            x, wt = _scaled(x, "x", 1, (-4, 4)), _scaled(wt, "w", 0, P.ROW_SCALES)
            dy = _scaled(dy, "dy", 1, P.ROW_SCALES)
        xd, wd, gd, bd, dyd, dresd = (t.to(DEV) for t in (x, wt, gam, bet, dy, dres))
        # forward
        ref = F.conv2d(_ln64(x, gam, bet), wt.double())
        f32 = P.rel_err_rows(F.conv2d(_ln32(x, gam, bet), wt), ref)
        with knobs(k24=1):
            y = ops.ln_conv1x1_forward(xd, gd, bd, wd)
        assert y is not None
        _note("ln_conv1x1_forward", P.rel_err_rows(y, ref), max(2 * f32, 1e-6))
        # weight gradient with the LayerNorm on load
        refw = dy.transpose(0, 1).reshape(k, -1).double() @ _ln64(x, gam, bet).transpose(0, 1).reshape(c, -1).t()
        xn32 = _ln32(x, gam, bet).transpose(0, 1).reshape(c, -1)
        f32w = P.rel_err_rows(dy.transpose(0, 1).reshape(k, -1) @ xn32.t(), refw, (0,))
        _, mean, rstd = ops.layernorm_forward(xd, gd, bd)
        with knobs(k25=1):
            dw = ops.conv1x1_wgrad_ln(dyd, xd, mean, rstd, gd, bd, wd)
        _note("conv1x1_wgrad_ln", P.rel_err_rows(dw.reshape(k, c), refw, (0,)), max(2 * f32w, 1e-6))
        # input gradient + LayerNorm backward
        outs = {}
        for dt in (torch.float64, torch.float32):
            xr = x.to(dt).requires_grad_(True)
            gr, br = gam.to(dt).requires_grad_(True), bet.to(dt).requires_grad_(True)
            ln = _ln64(xr, gr, br) if dt == torch.float64 else _ln32(xr, gr, br)
            F.conv2d(ln, wt.to(dt)).backward(dy.to(dt))
            outs[dt] = (xr.grad + dres.to(dt), gr.grad, br.grad)
        got = ops.conv1x1_dgrad_ln_backward(dyd, wd, xd, gd, mean, rstd, dres=dresd)
        assert got is not None
        for name, gv, r64, r32, dims in zip(("dx", "dgamma", "dbeta"), got, outs[torch.float64], outs[torch.float32],
                                            ((0, 1), (), ())):
            r64v, r32v, gvv = (r64, r32, gv) if dims else (r64.view(1, -1), r32.view(1, -1), gv.view(1, -1))
            dims = dims or (0,)
            bound = max(2 * P.rel_err_rows(r32v, r64v, dims), 1e-6)
            _note("conv1x1_dgrad_ln_backward %s" % name, P.rel_err_rows(gvv, r64v, dims), bound)


# ---------------------------------------------------------------------------------------------- dense 3x3
SHAPES_3X3 = [(3, 48, 128), (96, 3, 128), (48, 24, 128), (96, 48, 64), (192, 96, 32), (384, 768, 16), (192, 384, 32),
              (96, 192, 64), (64, 64, 64), (128, 128, 32), (320, 320, 16)]


def _conv_chain(b, m, k, side):
    """The k chain of one accumulator of a dense 3x3 convolution (M = m, K = 9 k): all 9 taps of the 16-padded channels, or
    that cut into the slices of a split over the stages (pir_conv3x3_x3_ws_floats = splits x b x m x h x w), as the knob 44
    setting in force plans it."""
    ws = _lib().pir_conv3x3_x3_ws_floats(b, m, k, side, side)
    sp = ws // (b * m * side * side) if ws else 1
    return -(-9 * (-(-k // 16) * 16) // sp)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("kind", ["uniform", "mixed"])
def test_dense_3x3_vs_float64(split, kind):
    """conv3x3_forward / conv3x3_dgrad, unsplit (knob 44 = 0) and split over their stages where the plan splits (knob 44 =
    1: pir_conv3x3_x3_ws_floats > 0), and conv3x3_wgrad, at every dense 3x3 shape of the network (batch 1)."""
    from promptir_amd import ops

    L = _lib()
    b, splits_seen = 1, 0
    for cin, cout, side in SHAPES_3X3:
        x, wt, dy = rnd("x", b, cin, side, side), rnd("w", cout, cin, 3, 3), rnd("dy", b, cout, side, side)
        if kind == "mixed":
            x, dy = _scaled(x, "x", 1, P.IN_SCALES), _scaled(dy, "dy", 1, P.IN_SCALES)
            wt = _scaled(wt, "w", 0 if cout > 3 else 1, P.ROW_SCALES)
        x64, w64, dy64 = x.double(), wt.double(), dy.double()
        xd, wd, dyd = x.to(DEV), wt.to(DEV), dy.to(DEV)
        with knobs(k44=split):
            fwd_split = L.pir_conv3x3_x3_ws_floats(b, cout, cin, side, side) > 0
            bwd_split = L.pir_conv3x3_x3_ws_floats(b, cin, cout, side, side) > 0
            fwd_chain, bwd_chain = _conv_chain(b, cout, cin, side), _conv_chain(b, cin, cout, side)
            y = ops.conv3x3_forward(xd, wd) if bool(split) == fwd_split else None
            dx = ops.conv3x3_dgrad(dyd, wd) if bool(split) == bwd_split else None
        tag = "split" if split else "unsplit"
        if y is not None:
            _note("3x3 fwd %s" % tag, P.rel_err_rows(y, F.conv2d(x64, w64, padding=1)), P.x3_bound(fwd_chain))
            splits_seen += split
        if dx is not None:
            _note("3x3 dgrad %s" % tag, P.rel_err_rows(dx, F.conv_transpose2d(dy64, w64, padding=1)),
                  P.x3_bound(bwd_chain))
            splits_seen += split
        if split == 0 and kind == "uniform":
            dw = ops.conv3x3_wgrad(dyd, xd, wd)
            ref = torch.nn.grad.conv2d_weight(x64, wt.shape, dy64, padding=1)
            nws = L.pir_conv3x3_wgrad_ws_floats(cout, cin, side, side, b)
            parts = max(1, int(nws) // (cout * cin * 9))
            chain = int(math.ceil(b * side * side / parts / 128.0) * 128)
            _note("3x3 wgrad", P.rel_err_rows(dw.reshape(cout, -1), ref.reshape(cout, -1), (0,)),
                  P.x3_bound(min(chain, b * side * side, 4096)))
    assert split == 0 or splits_seen > 0, "no shape ran split over its stages"


# ---------------------------------------------------------------------------------------------- fused GDFN forward
@pytest.mark.parametrize("b,c,h,w", [(1, 48, 32, 128), (2, 96, 16, 64)])
def test_gdfn_fused_forward_vs_float64(b, c, h, w, monkeypatch):
    """pir_gdfn_fused_fwd (its own term loop) vs float64 LayerNorm -> 1x1 -> depthwise 3x3 -> GELU gate; composite bar as
    for MDTA.  Measured on MI355X: <= 7.4e-7."""
    from promptir_amd import ops

    monkeypatch.setattr(ops, "GDFN_FUSED", True)
    hid = int(c * 2.66)
    x = rnd("x", b, c, h, w)
    lw, lb = 1 + 0.1 * rnd("lw", c), 0.1 * rnd("lb", c)
    win = rnd("win", 2 * hid, c, 1, 1) * (1.0 / c ** 0.5)
    wdw = rnd("wdw", 2 * hid, 1, 3, 3) * 0.3
    refs = {}
    for dt in (torch.float64, torch.float32):
        xn = _ln64(x, lw, lb) if dt == torch.float64 else _ln32(x, lw, lb)
        t = F.conv2d(F.conv2d(xn, win.to(dt)), wdw.to(dt), padding=1, groups=2 * hid)
        refs[dt] = F.gelu(t[:, :hid]) * t[:, hid:]
    g = ops.gdfn_fused_forward(x.to(DEV), lw.to(DEV), lb.to(DEV), win.to(DEV), wdw.to(DEV))
    assert g is not None, "shape not served"
    bound = max(2 * P.rel_err_rows(refs[torch.float32], refs[torch.float64]), 1e-6)
    _note("gdfn_fused_forward", P.rel_err_rows(g, refs[torch.float64]), bound)


# ---------------------------------------------------------------------------------------------- MDTA
def _mdta_ref(qkv, temp, dout, heads, dt):
    b, c3, h, w = qkv.shape
    C, c = c3 // 3, c3 // 3 // heads
    qr, tr = qkv.to(dt).requires_grad_(True), temp.to(dt).requires_grad_(True)
    q, k, v = (s.reshape(b, heads, c, h * w) for s in qr.split(C, dim=1))
    qn, kn = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    out = (torch.softmax(qn @ kn.transpose(-1, -2) * tr, dim=-1) @ v).reshape(b, C, h, w)
    out.backward(dout.to(dt))
    return out.detach(), qr.grad, tr.grad.view(1, -1)


@pytest.mark.parametrize("heads,c,hw,b", [(1, 48, 16384, 1), (2, 48, 4096, 2), (4, 48, 1024, 2), (8, 48, 256, 2),
                                          (2, 96, 1024, 2)])
def test_mdta_core_vs_float64(heads, c, hw, b, monkeypatch):
    """mdta_core_forward / mdta_core_backward with MDTA_DQK and SOFTMAX_PARTS on and off.  Composite (normalisation,
    softmax): at most 2x the error of PyTorch fp32 on the CPU, floor 1e-6.  The timed C ABI records confirm which kernels
    ran: pir_mdta_dqk with MDTA_DQK, pir_gemm_nt_partials with SOFTMAX_PARTS.
    Measured on MI355X: out <= 4.7e-7, dqkv <= 5.5e-7, dtemperature <= 5.4e-7."""
    from promptir_amd import ops

    C = heads * c
    h, w = hw // 64 if hw >= 64 else hw // 8, 64 if hw >= 64 else 8
    qkv, temp, dout = rnd("qkv", b, 3 * C, h, w), rnd("t", heads, 1, 1) * 0.5 + 1.0, rnd("do", b, C, h, w)
    r64 = _mdta_ref(qkv, temp, dout, heads, torch.float64)
    r32 = _mdta_ref(qkv, temp, dout, heads, torch.float32)
    bounds = [max(2 * P.rel_err_rows(a, b64, dims), 1e-6) for a, b64, dims in zip(r32, r64, ((0, 1), (0, 1), (0,)))]
    qd, td, dd = qkv.to(DEV), temp.to(DEV), dout.to(DEV)
    for dqk in (False, True):
        for parts in (False, True):
            monkeypatch.setattr(ops, "MDTA_DQK", dqk)
            monkeypatch.setattr(ops, "SOFTMAX_PARTS", parts)
            ops.lib.start_timing()
            try:
                og, attn, gram, sumsq = ops.mdta_core_forward(qd, td, heads)
                dqkv, dtemp = ops.mdta_core_backward(dd, qd, td, heads, attn, gram, sumsq)
            finally:
                ran = {name.split("@")[0] for name, *_ in ops.lib.stop_timing()}
            assert ("pir_mdta_dqk" in ran) == dqk, (dqk, sorted(ran))
            assert ("pir_gemm_nt_partials" in ran) == parts, (parts, sorted(ran))
            for name, got, ref, bound, dims in zip(("out", "dqkv", "dtemp"), (og, dqkv, dtemp.view(1, -1)), r64, bounds,
                                                  ((0, 1), (0, 1), (0,))):
                _note("mdta_core %s" % name, P.rel_err_rows(got, ref, dims), bound)


def _fold_ref(qkv, attn, wproj, x, dx1, heads, dt):
    b, c3, h, w = qkv.shape
    C, c = c3 // 3, c3 // 3 // heads
    vr = qkv[:, 2 * C:].to(dt).requires_grad_(True)
    ar, wr = attn.to(dt).requires_grad_(True), wproj.to(dt).requires_grad_(True)
    out = (ar @ vr.reshape(b, heads, c, h * w)).reshape(b, C, h * w)
    x1 = (wr @ out).reshape(b, C, h, w) + x.to(dt)
    x1.backward(dx1.to(dt))
    return x1.detach(), vr.grad, ar.grad.reshape(b * heads * c, c), wr.grad


@pytest.mark.parametrize("heads,c,side", [(1, 48, 128), (2, 48, 64)])
@pytest.mark.parametrize("b", [1, 4])
def test_mdta_fold_vs_float64(heads, c, side, b):
    """mdta_fold_forward / mdta_fold_backward (attn @ v folded into project_out, the 64^2 / 128^2 levels): x1, dv, dattn and
    the batch-summed dW_proj against float64 autograd of W_proj (attn v) + x; composite bar as for mdta_core.
    Measured on MI355X: x1 <= 1.6e-7, dv <= 4.8e-7, dattn <= 5.5e-7, dW_proj <= 9.1e-7."""
    from promptir_amd import ops

    C, hw = heads * c, side * side
    qkv, x, dx1 = rnd("qkv", b, 3 * C, side, side), rnd("x", b, C, side, side), rnd("dx1", b, C, side, side)
    attn = torch.softmax(rnd("a", b, heads, c, c) * 4, dim=-1).contiguous()
    wproj = rnd("wp", C, C) * (1.0 / C ** 0.5)
    r64 = _fold_ref(qkv, attn, wproj, x, dx1, heads, torch.float64)
    r32 = _fold_ref(qkv, attn, wproj, x, dx1, heads, torch.float32)
    qd, ad, wd, xd, dd = (t.to(DEV) for t in (qkv, attn, wproj, x, dx1))
    x1, weff = ops.mdta_fold_forward(qd, ad, wd, xd, heads)
    dqkv = torch.zeros(b, 3 * C, side, side, device=DEV)
    dattn, dwproj = ops.mdta_fold_backward(dd, qd, ad, weff, wd, heads, dqkv)
    got = (x1, dqkv[:, 2 * C:], dattn.reshape(b * heads * c, c), dwproj.reshape(C, C))
    for name, g, a64, a32 in zip(("x1", "dv", "dattn", "dW_proj"), got, r64, r32):
        dims = (0, 1) if g.dim() == 4 else (0,)
        bound = max(2 * P.rel_err_rows(a32, a64, dims), 1e-6)
        _note("mdta_fold %s" % name, P.rel_err_rows(g, a64, dims), bound)
    assert float(dqkv[:, :2 * C].abs().max()) == 0          # only the v third is written


# ---------------------------------------------------------------------------------------------- exactness at the edges
TIES = torch.tensor([1 + 2 ** -8, 1 + 2 ** -8 + 2 ** -16, -(1 + 2 ** -8), -(1 + 2 ** -8 + 2 ** -16)], dtype=torch.float32)


def _within(got, want, rel=2.0 ** -25):
    got, want = got.cpu().double(), want.cpu().double()
    bad = (got - want).abs() > rel * want.abs()
    assert not bool(bad.any()), (int(bad.sum()), float((got - want).abs().max()))


@pytest.mark.parametrize("family", list(FAMILIES_1X1))
def test_one_hot_activations_return_the_weights(family):
    """Pixel p selects input channel p mod K: y[:, :, p] = w[:, p mod K] through hi, mid and lo of the pre-split weight,
    element by element to 2^-25 relative; weights of every scale and the round-to-nearest-even ties."""
    from promptir_amd import ops

    ran = 0
    for cin, cout, side, b in ((48, 144, 16, 2), (96, 510, 16, 1), (192, 96, 32, 8), (510, 96, 32, 2), (384, 2042, 32, 1)):
        hw = side * side
        w = _scaled(rnd("w", cout, cin, 1, 1), "w", 1, (-20, 20))
        w.view(-1)[:4 * cout] = TIES.repeat(cout)
        x = torch.zeros(b, cin, hw)
        p = torch.arange(hw)
        x[:, p % cin, p] = 1.0
        x = x.reshape(b, cin, side, side)
        want = w.reshape(cout, cin)[:, p % cin].unsqueeze(0).expand(b, cout, hw)
        with knobs(**FAMILIES_1X1[family]):
            y = torch.empty(b, cout, side, side, device=DEV)
            xd, wd = x.to(DEV), w.to(DEV)
            if not _serves(family, _nn_desc(cout, cin, hw, b, False, wd, xd, y)):
                continue
            got = ops.conv1x1_forward(xd, wd)
        _within(got.reshape(b, cout, hw), want)
        ran += 1
    assert ran > 0


@pytest.mark.parametrize("family", list(FAMILIES_1X1))
def test_identity_weights_return_the_activations(family):
    """W = I: y = x and dx = dy through the activation-side split of each kernel's loader, element by element to 2^-25
    relative; mixed-scale activations and the round-to-nearest-even ties."""
    from promptir_amd import ops

    ran = 0
    for c, side, b in ((48, 128, 1), (96, 64, 2), (96, 32, 8), (192, 32, 2), (384, 16, 8), (510, 16, 1)):
        hw = side * side
        x = _scaled(rnd("x", b, c, side, side), "x", 1, (-20, 20))
        x.view(-1)[:4 * 64] = TIES.repeat(64)
        w = torch.eye(c).reshape(c, c, 1, 1)
        xd, wd = x.to(DEV), w.to(DEV)
        with knobs(**FAMILIES_1X1[family]):
            y = torch.empty(b, c, side, side, device=DEV)
            fwd = _serves(family, _nn_desc(c, c, hw, b, False, wd, xd, y))
            bwd = _serves(family, _nn_desc(c, c, hw, b, True, wd, xd, y))
            got_f = ops.conv1x1_forward(xd, wd) if fwd else None
            got_d = ops.conv1x1_dgrad(xd, wd) if bwd else None
        for got in (got_f, got_d):
            if got is not None:
                _within(got, x)
                ran += 1
    assert ran > 0


@pytest.mark.parametrize("b,c,h,w,split", [(1, 16, 1, 7, 0), (2, 24, 2, 9, 0), (1, 48, 5, 13, 0), (1, 96, 3, 33, 0),
                                             (1, 384, 1, 7, 1), (1, 192, 2, 9, 1), (1, 256, 3, 11, 1)])
def test_dense_3x3_one_hot_tap_is_a_shift(b, c, h, w, split):
    """An identity over channels at one of the 9 taps shifts the image: exact (2^-25 relative) and exact zeros in the
    padded border, forward and input gradient, odd widths, heights 1 and 2; unsplit, and split over the stages (knob 44
    = 1) on shapes whose plan splits."""
    from promptir_amd import ops

    with knobs(k44=split):
        assert (_lib().pir_conv3x3_x3_ws_floats(b, c, c, h, w) > 0) == bool(split)

    x = _scaled(rnd("x", b, c, h, w), "x", 1, (-20, 20))
    x.view(-1)[:4 * 4] = TIES.repeat(4)
    xd = x.to(DEV)
    for tap in range(9):
        ty, tx = divmod(tap, 3)
        wt = torch.zeros(c, c, 3, 3)
        wt[torch.arange(c), torch.arange(c), ty, tx] = 1.0
        want_f = F.conv2d(x.double(), wt.double(), padding=1)
        want_d = F.conv_transpose2d(x.double(), wt.double(), padding=1)
        with knobs(k44=split):
            got_f = ops.conv3x3_forward(xd, wt.to(DEV))
            got_d = ops.conv3x3_dgrad(xd, wt.to(DEV))
        for got, want in ((got_f, want_f), (got_d, want_d)):
            _within(got, want)
            assert bool((got.cpu()[want == 0] == 0).all()), tap


def test_split_ties_through_a_full_product():
    """Operands 1 + 2^-8 (rounds to even: h = 1) and 1 + 2^-8 + 2^-16 (rounds up, the mid piece changes sign) and their
    negatives on both sides of a product, against float64."""
    from promptir_amd import ops

    cin, cout, side = 16, 32, 16
    x = TIES[torch.arange(cin * side * side) % 4].reshape(1, cin, side, side)
    w = TIES[(torch.arange(cout * cin) * 3 + 1) % 4].reshape(cout, cin, 1, 1)
    got = ops.conv1x1_forward(x.to(DEV), w.to(DEV))
    ref = F.conv2d(x.double(), w.double())
    assert P.rel_err_rows(got, ref) <= P.x3_bound(cin)


def test_zz_print_measured():
    """(runs last in the file) the largest row-normalised error per family measured above."""
    for k in sorted(MEASURED):
        print("measured %-40s %.3e" % (k, MEASURED[k]))
